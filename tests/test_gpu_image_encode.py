"""Float maps become image samples on the device (pbr_pack_images; csrc/pack_image.hip) -- MaterialBase.to_pil, base.py:793-850, as one
launch per map size -- and travel home as samples.  The host oracle is tools/gen_export_golden.restate, the numpy fp32 restatement of
upstream's operation order that tests/test_export_host.py pins on tests/golden/export.npz (outputs of the real reference): every
comparison here is for EQUALITY."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_export_golden as G  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import _upload as U  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402
from pypbr_amd import io as pio  # noqa: E402
from pypbr_amd.blending import HeightBlend  # noqa: E402
from pypbr_amd.materials import BasecolorMetallicMaterial  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "export.npz"))
TILES = os.path.join(ROOT, "tests", "golden", "tiles")
DTYPE = {8: np.uint8, 16: np.uint16}


def pack(t, bits=8, normal=False):
    """pack_image of a host array / tensor on the device -> numpy (H,W,C)."""
    t = torch.as_tensor(t)
    return F.pack_image(t.cuda() if not t.is_cuda else t, bits, normal).cpu().numpy()


def check(t, bits=8, normal=False):
    got, want = pack(t, bits, normal), G.restate(torch.as_tensor(t).cpu().numpy(), bits, normal)
    assert got.dtype == DTYPE[bits] and got.shape == want.shape
    assert np.array_equal(got, want), (tuple(want.shape), bits, normal, int((got != want).sum()))
    return got


def unit_normals(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(3, h, w, generator=g)
    n = n / n.norm(dim=0, keepdim=True)
    special = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [-(3 ** -0.5)] * 3]).t()
    k = min(special.shape[1], h * w)
    n.view(3, -1)[:, :k] = special[:, :k]
    return n


def neighbours(v, steps):
    """The float32 values `steps` ulps either side of every element of v, v itself in the middle: (2 * steps + 1, len(v))."""
    rows, lo, hi = [v], v, v
    for _ in range(steps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        rows = [lo] + rows + [hi]
    return np.stack(rows).astype(np.float32)


# ---- layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", [(24, 256), (24, 250), (37, 3), (1, 1), (1, 5), (5, 1)])
def test_every_form_writes_dense_hwc_samples(h, w):
    """24 x 256 takes the dense form (4 pixels a lane, whole dwords), every other shape the general one; several blocks at 24 x 256."""
    g = torch.Generator().manual_seed(h * 1000 + w)
    for channels in (1, 2, 3, 4):
        t = torch.rand(channels, h, w, generator=g)
        for bits in (8, 16):
            check(t, bits)
    out = torch.empty(h, w, 3, dtype=torch.uint8, device="cuda")
    t = torch.rand(3, h, w, generator=g)
    assert F.pack_image(t.cuda(), out=out) is out and np.array_equal(out.cpu().numpy(), G.restate(t.numpy()))
    half = torch.rand(3, h, w, generator=g).half()                    # a float16 map is converted to float32 first
    assert np.array_equal(pack(half), G.restate(half.float().numpy()))
    assert np.array_equal(F.pack_image(t).numpy(), G.restate(t.numpy()))       # a CPU tensor: staged through the device


# ---- every level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_all_256_levels_and_the_floats_where_truncation_flips(channels):
    levels = (np.arange(256, dtype=np.float32) / np.float32(255))
    rng = np.random.default_rng(channels)
    for shape in ((1, 256), (64, 4), (2, 128), (256, 1), (4, 64)):    # dense forms and general ones (one pixel a row; width 1)
        perm = np.stack([rng.permutation(256) for _ in range(channels)])
        got = pack(levels[perm].reshape((channels,) + shape))
        assert np.array_equal(got.reshape(256, channels).T, perm), shape         # k / 255 gives k back
    around = neighbours(levels, 2)                                               # (5, 256): two ulps below ... two ulps above
    t = np.stack([around[:, rng.permutation(256)] for _ in range(channels)])     # (C, 5, 256)
    check(t)                                                                     # dense
    check(np.ascontiguousarray(t[:, :, :250]))                                   # ragged
    check(np.ascontiguousarray(t.reshape(channels, 256, 5)))


@pytest.mark.parametrize("width", [256, 255])
def test_all_65536_levels_and_their_neighbours(width):
    levels = (np.arange(65536, dtype=np.float32) / np.float32(65535))
    rows = -(-65536 // width)
    t = np.zeros(rows * width, dtype=np.float32)
    t[:65536] = levels
    got = pack(t.reshape(1, rows, width), 16)
    assert np.array_equal(got.reshape(-1)[:65536], np.arange(65536))             # k / 65535 gives k back
    assert np.array_equal(got, G.restate(t.reshape(1, rows, width), 16))
    around = neighbours(levels, 1).reshape(-1)                                   # 3 x 65536
    rows = -(-around.size // width)
    t = np.zeros(rows * width, dtype=np.float32)
    t[:around.size] = around
    check(t.reshape(1, rows, width), 16)


# ---- outside [0, 1] -------------------------------------------------------------------------------------------------------------------
def test_values_outside_the_unit_interval_saturate_and_nan_gives_zero():
    special = np.array([-0.0, -1e-7, np.nextafter(np.float32(1), np.float32(2)), 2.0, 1e30, np.inf, -np.inf, np.nan, 1e-40], dtype=np.float32)
    want = {8: [0, 0, 255, 255, 255, 255, 0, 0, 0], 16: [0, 0, 65535, 65535, 65535, 65535, 0, 0, 0]}
    for shape in ((3, 4), (3, 3), (1, 9), (9, 1)):                               # 3 x 4 + padding: dense; the others general
        for channels in (1, 3):
            t = np.full((channels,) + shape, 0.25, dtype=np.float32)
            n = min(special.size, shape[0] * shape[1])
            t.reshape(channels, -1)[:, :n] = special[:n]
            for bits in (8, 16):
                got = check(t, bits)
                assert got.reshape(-1, channels)[:n, 0].tolist() == want[bits][:n], (shape, channels, bits)
            if channels == 3:
                check(t, 8, normal=True)                                        # NaN and the infinities through (n + 1) * 0.5 too


# ---- the normal map -------------------------------------------------------------------------------------------------------------------
def test_normal_encode_dense_ragged_and_strided():
    for h, w, seed in ((24, 256, 1), (24, 250, 2), (37, 3, 3), (1, 1, 4), (1, 5, 5), (5, 1, 6)):
        check(unit_normals(h, w, seed), 8, normal=True)
    check(unit_normals(24, 256, 7), 16, normal=True)
    check(unit_normals(24, 250, 8), 16, normal=True)
    # a view into a block whose plane pitch is larger than H * W: a multiple of 4 elements (dense form) and not (general form)
    h, w = 24, 256
    n = unit_normals(h, w, 9)
    want = G.restate(n.numpy(), 8, True)
    for pitch in (h * w + 64, h * w + 3):
        block = torch.full((3 * pitch + 8,), 7.0, device="cuda")
        view = block.as_strided((3, h, w), (pitch, w, 1), 4)
        view.copy_(n)
        keep = block.clone()
        assert np.array_equal(F.pack_image(view, 8, True).cpu().numpy(), want), pitch
        assert torch.equal(block, keep)
    # a crop view: a row pitch
    big = unit_normals(30, 48, 10).cuda()
    crop = big[:, 3:27, 5:42]
    assert not crop.is_contiguous()
    assert np.array_equal(F.pack_image(crop, 8, True).cpu().numpy(), G.restate(crop.cpu().numpy(), 8, True))
    wide = unit_normals(30, 48, 11).cuda()[:, 3:27, 8:40]                        # width 32, 16-byte aligned rows, yet a row pitch: general
    assert np.array_equal(F.pack_image(wide, 8, True).cpu().numpy(), G.restate(wide.cpu().numpy(), 8, True))


def test_golden_maps_give_the_references_samples():
    """The floats the reference held -> the samples the reference's to_pil made of them."""
    for h, w in G.SIZES:
        s = G.size_key(h, w)
        assert np.array_equal(pack(GOLD["nrm__" + s], 8, True), GOLD["pil8__normal__" + s]), s
        assert np.array_equal(pack(GOLD["in__albedo__" + s]), GOLD["pil8__albedo__" + s]), s
        for name in ("roughness", "height", "metallic"):
            assert np.array_equal(pack(GOLD["in__%s__%s" % (name, s)])[:, :, 0], GOLD["pil8__%s__%s" % (name, s)]), (s, name)
        assert np.array_equal(pack(GOLD["in__height__" + s], 16)[:, :, 0], GOLD["pil16__height__" + s]), s


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def _five_maps(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return {"albedo": torch.rand(3, h, w, generator=g).cuda(), "normal": unit_normals(h, w, seed + 1).cuda(),
            "roughness": torch.rand(1, h, w, generator=g).cuda(), "metallic": torch.rand(1, h, w, generator=g).cuda(),
            "height": torch.rand(1, h, w, generator=g).cuda()}


@pytest.mark.parametrize("h, w", [(24, 256), (24, 250)])
def test_one_call_with_five_maps_equals_five_calls(h, w):
    maps = _five_maps(h, w, 40)
    bits = {"albedo": 8, "normal": 8, "roughness": 8, "metallic": 8, "height": 16}
    outs = {k: torch.zeros(h, w, t.shape[0], dtype=torch.uint8 if bits[k] == 8 else torch.uint16, device="cuda") for k, t in maps.items()}
    rows = [U._image_pack(maps[k], outs[k].data_ptr(), bits[k], k == "normal") for k in maps]
    U._pack_images_call(maps["albedo"].device, rows, h, w)
    for k, t in maps.items():
        single = F.pack_image(t, bits[k], k == "normal")
        assert torch.equal(outs[k], single), k
        assert np.array_equal(single.cpu().numpy(), G.restate(t.cpu().numpy(), bits[k], k == "normal")), k


def test_download_samples_is_one_abi_call_per_size_and_one_copy(monkeypatch):
    lib = N.lib()
    real, real_to_host, calls, copies = lib.pbr_pack_images, U.to_host, [], []

    def counting(table, n, h, w, stream):
        calls.append((n, h, w))
        return real(table, n, h, w, stream)

    def counting_to_host(t, *a):
        copies.append(t.numel())
        return real_to_host(t, *a)
    monkeypatch.setattr(lib, "pbr_pack_images", counting)
    monkeypatch.setattr(U, "to_host", counting_to_host)
    maps = _five_maps(24, 256, 50)
    got = F.download_samples(maps, {"height": 16})
    assert calls == [(5, 24, 256)] and len(copies) == 1
    assert list(got) == list(maps)
    for k, t in maps.items():
        assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], G.restate(t.cpu().numpy(), 16 if k == "height" else 8, k == "normal")), k
    roots = []
    for a in got.values():                                                       # views of ONE block, no per-map copy
        assert not a.flags.owndata
        while isinstance(a.base, np.ndarray):
            a = a.base
        roots.append(a)
    assert all(r is roots[0] for r in roots)
    del calls[:], copies[:]
    mixed = dict(maps)
    mixed["height"] = torch.rand(1, 37, 53).cuda()
    mixed["extra"] = torch.rand(3, 37, 53).cuda()
    got = F.download_samples(mixed, 8)
    assert sorted(calls) == [(2, 37, 53), (4, 24, 256)] and len(copies) == 1
    assert np.array_equal(got["extra"], G.restate(mixed["extra"].cpu().numpy()))


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
def test_nothing_outside_a_maps_samples_is_written(bits):
    """Every destination sits between sentinel bytes; width 256 runs in the dense form and, from a source that is not 16-byte aligned or
    into a destination that is not dword aligned, in the general one; the other widths are general by their width."""
    esz, guard = bits // 8, 512
    g = torch.Generator().manual_seed(bits)
    for h in (1, 24):
        for w in (1, 2, 3, 5, 250, 256):
            for channels in (1, 3, 4):
                for src_shift, dst_shift in ((0, 0), (1, 0), (0, esz)) if w == 256 else ((0, 0), (0, esz)):
                    store = torch.rand(channels * h * w + 4, generator=g).cuda()
                    src = store[src_shift:src_shift + channels * h * w].view(channels, h, w)
                    keep = store.clone()
                    nbytes = h * w * channels * esz
                    arena = torch.full((2 * guard + nbytes + 8,), 0xA5, dtype=torch.uint8, device="cuda")
                    lo = guard + dst_shift
                    row = U._image_pack(src, arena.data_ptr() + lo, bits, False)
                    U._pack_images_call(src.device, [row], h, w)
                    host = arena.cpu().numpy()
                    case = (h, w, channels, src_shift, dst_shift)
                    assert (host[:lo] == 0xA5).all() and (host[lo + nbytes:] == 0xA5).all(), case
                    got = host[lo:lo + nbytes].copy().view(DTYPE[bits]).reshape(h, w, channels)
                    assert np.array_equal(got, G.restate(src.cpu().numpy(), bits)), case
                    assert torch.equal(store, keep), case


# ---- material level -------------------------------------------------------------------------------------------------------------------
CROP = (100, 200, 100 + 52, 200 + 48)                                            # left, top, right, bottom: 48 rows x 52 columns


def _crops(height8=False):
    out = {}
    for name, mode in (("basecolor", "RGB"), ("normal", "RGB"), ("roughness", "L"), ("metallic", "L"), ("height", None)):
        with Image.open(os.path.join(TILES, name + ".png")) as im:
            c = im.crop(CROP)
            out[name] = c.convert(mode) if mode else c
            out[name].load()
    assert out["height"].mode == "I;16"
    if height8:
        out["height"] = Image.fromarray((np.array(out["height"], dtype=np.uint16) >> 8).astype(np.uint8))
    return out


def _material(crops):
    return BasecolorMetallicMaterial(albedo=crops["basecolor"], normal=crops["normal"], roughness=crops["roughness"],
                                     metallic=crops["metallic"], height=crops["height"]).to("cuda")


def _expect(material, wide=()):
    return {k: G.restate(t.cpu().numpy(), 16 if k in wide else 8, k == "normal") for k, t in material._raw.items()}


def _assert_images(pil, want, wide=()):
    assert list(pil) == list(want)
    for k, im in pil.items():
        a = want[k]
        assert im.size == (a.shape[1], a.shape[0]), k
        assert im.mode == ("I;16" if k in wide else "RGB" if a.shape[2] == 3 else "L"), (k, im.mode)
        got = np.array(im)
        assert got.dtype == a.dtype and np.array_equal(got.reshape(a.shape), a), k


def test_material_to_pil_on_the_device():
    crops = _crops()
    m = _material(crops)
    before = dict(m._raw)
    assert list(before) == ["albedo", "normal", "roughness", "height", "metallic"] and all(t.is_cuda for t in before.values())
    pil = m.to_pil()
    assert [im.mode for im in pil.values()] == ["RGB", "RGB", "L", "L", "L"] and all(im.size == (52, 48) for im in pil.values())
    for name, key in (("albedo", "basecolor"), ("roughness", "roughness"), ("metallic", "metallic")):
        assert np.array_equal(np.array(pil[name]), np.array(crops[key])), name   # an image's samples come back exactly
    _assert_images(pil, _expect(m))                                              # the normal map and the 16-bit height: the restatement
    deep = m.to_pil({"height": "I;16", "albedo": "CMYK"})
    assert [im.mode for im in deep.values()] == ["RGB", "RGB", "L", "I;16", "L"]
    got = np.array(deep["height"])
    assert got.dtype == np.uint16 and np.array_equal(got, np.array(crops["height"]))
    _assert_images(deep, _expect(m, ("height",)), ("height",))
    assert all(m._raw[k] is t and m._raw[k].device == t.device for k, t in before.items())
    arrays = m.to_numpy()
    assert all(np.array_equal(arrays[k], t.cpu().numpy()) for k, t in before.items())
    with pytest.raises(ValueError):
        m.to_pil({"normal": "I;16"})
    # off the 1/255 grid: after a resize, and after a blend
    m.resize((40, 44))
    _assert_images(m.to_pil({"height": "I;16"}), _expect(m, ("height",)), ("height",))
    other = _material(_crops()).resize((40, 44)).roll((7, 11))
    blended, _ = HeightBlend(blend_width=0.2)(m, other)
    pil = blended.to_pil()
    _assert_images(pil, _expect(blended))
    assert pil["albedo"].size == (44, 40)


def test_cpu_home_material_goes_up_packed_and_comes_back_as_samples():
    crops = _crops()
    m = BasecolorMetallicMaterial(albedo=crops["basecolor"], normal=crops["normal"], roughness=crops["roughness"],
                                  metallic=crops["metallic"], height=crops["height"])
    assert m.device.type == "cpu" and all(F.is_encoded(t) for t in m._raw.values())
    pil = m.to_pil()                                                             # normal and the 16-bit height through the device
    for name, key in (("albedo", "basecolor"), ("roughness", "roughness"), ("metallic", "metallic")):
        assert np.array_equal(np.array(pil[name]), np.array(crops[key])), name
    _assert_images(pil, _expect(m))
    floats = BasecolorMetallicMaterial(albedo=torch.rand(3, 9, 7), roughness=torch.rand(1, 9, 7))
    before = dict(floats._raw)
    _assert_images(floats.to_pil(), _expect(floats))
    assert all(floats._raw[k] is t for k, t in before.items())                  # host maps stay the material's maps


def test_round_trip_through_disk(tmp_path):
    crops = _crops(height8=True)
    m = _material(crops)
    want_normal = G.restate(m.normal.cpu().numpy(), 8, True)
    m.save_to_folder(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == list(GOLD["files__default"])
    with Image.open(tmp_path / "normal.png") as im:
        assert im.mode == "RGB" and np.array_equal(np.array(im), want_normal)
    back = pio.load_material_from_folder(str(tmp_path)).to("cuda")
    assert type(back) is BasecolorMetallicMaterial
    for name in ("albedo", "roughness", "height", "metallic"):
        assert torch.equal(back._raw[name], m._raw[name]), name                 # bit-equal floats
