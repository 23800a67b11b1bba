"""Photometric-stereo initialisation on the host side (no GPU): the numpy oracle of the definition (tools/photometric_oracle.py) equals
numpy's least squares and recovers exactly Lambertian data; the populations the GPU tests run on (tools/photometric_cases.py) hold what
those tests need; the C ABI declares and exports pbr_photometric_stereo (ABI still 9) and returns every caller-error code before any
device work; the Python surface raises ValueError for every bad argument.

Population counts, recorded from the float64 oracle at the defaults (K = 3, tau = 0.1, kappa = 1e-4), 24 x 36 | 24 x 35:
  set        observations in attached shadow   valid / invalid   margin < 1e-4   valid with c >= 0.05   smallest valid c
  gentle     0.58 % | 0.58 %                   864 / 0 | 840 / 0     1 | 0           100 % | 100 %          0.312 | 0.313
  shadowed   16.6 % | 16.6 %                   863 / 1 | 839 / 1     3 | 0           99.8 % | 99.5 %        0.044 | 0.040
  partial    0.58 % | 0.58 %                   588 / 276 | 567 / 273 1 | 0           100 % | 100 %          0.177 | 0.174
(`partial`: 68 % valid; 264 pixels see fewer than three shots and fail at the first solve, 12 | 9 fail at the second.)  Required of every
set: at most 2 % of the pixels with margin < 1e-4, at least 90 % of the valid pixels with c >= 0.05.

On exactly Lambertian linear data in float64, share of the `shadowed` pixels more than 0.01 degrees off after K = 1 / 2 / 3 solves:
50.5 % / 8.7 % / 0 % (24 x 36): the reweighting passes are what recovers a surface with attached shadows.

float32 against float64, the oracle itself (max over the banded pixels -- valid, margin >= 1e-4, c >= 0.05 -- of normal, albedo,
confidence), and the band the GPU test holds the kernel to: 4 x that error (hardware rsqrt, rcp, log2 and exp2 at about 1 ulp each and
fused multiply-adds, where numpy float32 rounds every operation correctly), covered by the smallest of 2e-6, 1e-5, 1e-4:
  gentle     4.0e-7 | 4.3e-7   -> 2e-6 | 2e-6
  shadowed   1.3e-6 | 2.1e-6   -> 1e-5 | 1e-5
  partial    4.7e-7 | 6.7e-7   -> 2e-6 | 1e-5
  rendered   (host render) 4.0e-7 -> 2e-6"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import photometric_cases as C  # noqa: E402
import photometric_oracle as O  # noqa: E402

import abi_header  # noqa: E402
from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import capture  # noqa: E402

NAMES = ("gentle", "shadowed", "partial")
SIZES = (C.SIZE, C.SIBLING)


@functools.lru_cache(maxsize=None)
def case(name, size=C.SIZE, encode=True):
    return C.lambertian(name, size, encode)


@functools.lru_cache(maxsize=None)
def solved(name, size=C.SIZE, dtype=np.float64, **kw):
    c = case(name, size)
    return O.photometric_stereo(c.targets, c.weights, c.light, c.intensity, light_size=C.LIGHT_SIZE, dtype=dtype, **kw)


def angle_deg(a, b):
    return np.degrees(np.arccos(np.clip((a * b).sum(axis=0), -1.0, 1.0)))


# ---------------------------------------------------------------- the oracle against numpy
def test_one_pass_equals_numpy_least_squares():
    c = case("gentle", encode=False)
    r = O.photometric_stereo(c.targets, None, c.light, c.intensity, light_size=C.LIGHT_SIZE, targets_srgb=False, iterations=1)
    w, att = O.geometry(c.light, C.SIZE, "point", C.LIGHT_SIZE)
    y = (c.targets / (c.intensity[None, :, None, None] * att[:, None])).mean(axis=1)              # [L,H,W]
    worst = 0.0
    for (py, px) in np.ndindex(*C.SIZE):
        g = np.linalg.lstsq(w[:, :, py, px], y[:, py, px], rcond=None)[0]
        worst = max(worst, np.abs(g - r.g[:, py, px]).max())
    print("one pass against np.linalg.lstsq: %.2e" % worst)
    assert r.valid.all() and worst <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_lambertian_data_are_recovered_where_no_shot_is_shadowed(name):
    c = case(name, encode=False)
    r = O.photometric_stereo(c.targets, c.weights, c.light, c.intensity, light_size=C.LIGHT_SIZE, targets_srgb=False)
    lit = ~c.shadowed.any(axis=0) & r.valid
    e_n, e_a = np.abs(r.normal - c.normal)[:, lit].max(), np.abs(r.albedo - c.albedo)[:, lit].max()
    print("%s: %d unshadowed valid pixels, |normal| %.2e |albedo| %.2e" % (name, int(lit.sum()), e_n, e_a))
    assert lit.sum() >= 400 and e_n <= 1e-9 and e_a <= 1e-9
    # and the albedo is the mean-free one: every channel, not the grey mean the solve uses
    assert np.abs(r.albedo[0] - r.albedo[1])[lit].max() > 0.1


def test_reweighting_passes_recover_the_shadowed_surface():
    c = case("shadowed", encode=False)
    off = []
    for K in (1, 2, 3):
        r = O.photometric_stereo(c.targets, None, c.light, c.intensity, light_size=C.LIGHT_SIZE, targets_srgb=False, iterations=K)
        off.append(float((angle_deg(r.normal, c.normal)[r.valid] > 0.01).mean()))
    print("shadowed, share more than 0.01 degrees off after 1 / 2 / 3 solves: %.3f / %.3f / %.3f" % tuple(off))
    assert off[0] > 0.4 and 0.02 < off[1] < 0.15 and off[2] <= 0.005


def test_invalid_pixels_and_zero_weights():
    c = case("partial")
    r = solved("partial")
    seen = (c.weights != 0).sum(axis=0)
    assert (~r.valid[seen < 3]).all() and r.valid[seen >= 4].mean() > 0.95
    inv = ~r.valid
    assert (r.normal[:, inv] == np.array([0.0, 0.0, 1.0])[:, None]).all() and (r.confidence[inv] == 0).all() and (r.confidence[r.valid] > 0).all()
    assert (r.albedo[:, seen == 0] == 0).all() and (seen == 0).sum() >= 48
    one = inv & (seen >= 1)
    assert (r.albedo[:, one].max(axis=0) > 0).mean() > 0.9                          # an invalid pixel still gets an albedo, from all its shots under the flat normal
    # a NaN target under a zero weight changes nothing
    t = c.targets.copy()
    t[np.broadcast_to((c.weights == 0)[:, None], t.shape)] = np.nan
    again = O.photometric_stereo(t, c.weights, c.light, c.intensity, light_size=C.LIGHT_SIZE)
    for a, b in zip(r[:4], again[:4]):
        assert np.array_equal(a, b)
    # fewer than three shots: rank < 3
    for L in (1, 2):
        few = O.photometric_stereo(case("gentle").targets[:L], None, c.light[:L], c.intensity, light_size=C.LIGHT_SIZE)
        assert not few.valid.any() and (few.confidence == 0).all()


# ---------------------------------------------------------------- the populations of the GPU tests
EXPECTED = {    # (name, width) -> (valid, invalid, pixels with margin < 1e-4)
    ("gentle", 36): (864, 0, 1), ("gentle", 35): (840, 0, 0),
    ("shadowed", 36): (863, 1, 3), ("shadowed", 35): (839, 1, 0),
    ("partial", 36): (588, 276, 1), ("partial", 35): (567, 273, 0),
}
FLOAT32_ERROR = {   # (name, width) -> the oracle's float32-against-float64 error on the banded pixels (recorded; asserted within 25 %)
    ("gentle", 36): 4.0e-7, ("gentle", 35): 4.3e-7, ("shadowed", 36): 1.3e-6, ("shadowed", 35): 2.1e-6,
    ("partial", 36): 4.7e-7, ("partial", 35): 6.7e-7,
}
BANDS = (2e-6, 1e-5, 1e-4)


def band_for(error):
    return next(b for b in BANDS if 4 * error <= b)


def float32_error(r32, r64):
    _, _, banded = C.classes(r64)
    return max(np.abs(r32.normal.astype(np.float64) - r64.normal)[:, banded].max(), np.abs(r32.albedo.astype(np.float64) - r64.albedo)[:, banded].max(),
               np.abs(r32.confidence.astype(np.float64) - r64.confidence)[banded].max())


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_populations_hold_what_the_gpu_tests_compare(name, size):
    assert C.SIZE == (24, 36) and C.SIBLING == (24, 35) and C.N_LIGHTS == 8
    c, r = case(name, size), solved(name, size)
    assert c.targets.dtype == np.float32 and c.targets.shape == (8, 3) + size and 0 <= c.targets.min() and c.targets.max() < 1
    clear, invalid_clear, banded = C.classes(r)
    valid, invalid, unclear = int(r.valid.sum()), int((~r.valid).sum()), int((~clear).sum())
    well = float((r.confidence[r.valid] >= C.WELL_CONDITIONED).mean())
    print("%s %s: shadowed %.4f  valid %d invalid %d  margin < 1e-4: %d  c >= 0.05: %.4f of the valid  min valid c %.4f  banded %d"
          % (name, size, c.shadowed.mean(), valid, invalid, unclear, well, r.confidence[r.valid].min(), int(banded.sum())))
    assert (valid, invalid, unclear) == EXPECTED[(name, size[1])]
    assert unclear <= 0.02 * r.valid.size and well >= 0.90
    if name == "shadowed":
        assert 0.10 <= c.shadowed.mean() <= 0.30
    if name == "partial":
        assert 0.6 <= valid / r.valid.size <= 0.8 and int(invalid_clear.sum()) >= 250
    # the float32 oracle: the same decisions wherever there is margin, and the error the GPU test's band is made from
    r32 = solved(name, size, np.float32)
    assert np.array_equal(r32.valid[clear], r.valid[clear])
    err = float32_error(r32, r)
    print("   float32 oracle against float64: %.2e -> band %.0e" % (err, band_for(err)))
    assert err <= 1.25 * FLOAT32_ERROR[(name, size[1])] and band_for(err) == band_for(FLOAT32_ERROR[(name, size[1])])


@functools.lru_cache(maxsize=None)
def rendered():
    """The gentle maps as a rough dielectric under the eight lights, from the committed torch oracle in float64: sRGB targets [L,3,H,W]."""
    import torch_oracle
    c = case("gentle")
    maps = dict(albedo=torch.from_numpy(c.albedo), normal=torch.from_numpy(c.normal), roughness=torch.full((1,) + C.SIZE, C.ROUGHNESS, dtype=torch.float64),
                metallic=torch.zeros((1,) + C.SIZE, dtype=torch.float64))

    def stack(albedo, normal, roughness, metallic, albedo_is_srgb):
        return torch.stack([torch_oracle.cook_torrance(albedo, normal, roughness, metallic, view=torch.tensor([0.0, 0.0, 1.0]),
                                                       light=torch.from_numpy(c.light[l]), intensity=torch.from_numpy(c.intensity), light_type="point",
                                                       light_size=C.LIGHT_SIZE, albedo_is_srgb=albedo_is_srgb) for l in range(C.N_LIGHTS)])
    return stack, maps, stack(albedo_is_srgb=False, **maps)


def test_rendered_set_a_rough_dielectric_is_close_to_lambertian():
    stack, maps, targets = rendered()
    c = case("gentle")
    t32 = targets.numpy().astype(np.float32)
    assert t32.max() < 1.0                                                          # nothing clipped
    r = O.photometric_stereo(t32, None, c.light, c.intensity, light_size=C.LIGHT_SIZE)
    r32 = O.photometric_stereo(t32, None, c.light, c.intensity, light_size=C.LIGHT_SIZE, dtype=np.float32)
    clear, _, banded = C.classes(r)
    err = float32_error(r32, r)
    median = float(np.median(angle_deg(r.normal, c.normal)))
    print("rendered: valid %d, margin < 1e-4: %d, banded %d, median angle %.3f degrees, float32 oracle %.2e -> band %.0e"
          % (int(r.valid.sum()), int((~clear).sum()), int(banded.sum()), median, err, band_for(err)))
    assert r.valid.all() and (~clear).sum() <= 0.02 * clear.size and banded.sum() >= 0.9 * clear.size
    assert median < 1.0 and err <= 1.25 * 4.0e-7 and band_for(err) == 2e-6
    # the stack loss at the photometric-stereo start against the flat grey start (float64, the oracle's render)
    start = stack(torch.from_numpy(O.linear_to_srgb(r.albedo)), torch.from_numpy(r.normal), maps["roughness"], maps["metallic"], True)
    flat_n = torch.zeros((3,) + C.SIZE, dtype=torch.float64)
    flat_n[2] = 1.0
    flat = stack(torch.full((3,) + C.SIZE, 0.5, dtype=torch.float64), flat_n, maps["roughness"], maps["metallic"], True)
    at_start, at_flat = float(((start - targets) ** 2).mean()), float(((flat - targets) ** 2).mean())
    print("rendered: stack loss %.3e at the start, %.3e at flat grey: %.0f x" % (at_start, at_flat, at_flat / at_start))
    assert at_flat >= 100 * at_start


def test_options_of_the_oracle():
    c = case("gentle")
    r = solved("gentle")
    enc = solved("gentle", albedo_srgb=True)
    assert np.array_equal(enc.albedo, O.linear_to_srgb(r.albedo)) and np.array_equal(enc.normal, r.normal)
    lin = O.srgb_to_linear(c.targets.astype(np.float64))
    plain = O.photometric_stereo(lin, None, c.light, c.intensity, light_size=C.LIGHT_SIZE, targets_srgb=False)
    assert np.abs(plain.normal - r.normal).max() <= 1e-12
    # a shared plane of weights scales A and b alike: the same solution
    half = O.photometric_stereo(c.targets, np.full(C.SIZE, 0.5), c.light, c.intensity, light_size=C.LIGHT_SIZE)
    assert np.abs(half.normal - r.normal).max() <= 1e-12 and np.abs(half.albedo - r.albedo).max() <= 1e-12
    # directional lights: no grid, no attenuation
    n = c.normal
    dirs = c.light / np.linalg.norm(c.light, axis=1, keepdims=True)
    flat = np.maximum((dirs[:, :, None, None] * n[None]).sum(axis=1), 0)[:, None] * c.albedo[None] / np.pi * 2.0
    d = O.photometric_stereo(flat, None, 3.0 * dirs, np.full(3, 2.0), light_type="directional", targets_srgb=False)
    lit = ~(flat[:, 0] == 0).any(axis=0) & d.valid
    assert lit.sum() > 400 and np.abs(d.normal - n)[:, lit].max() <= 1e-6 and np.abs(d.albedo - c.albedo)[:, lit].max() <= 1e-6    # (unit directions travel as float32)


# ---------------------------------------------------------------- the ABI surface
def test_header_declares_and_library_exports_the_entry_point():
    raw = abi_header.RAW
    assert "#define PBR_MAX_PHOTOMETRIC_SHOTS 16" in raw and N.MAX_PHOTOMETRIC_SHOTS == 16
    assert N.ABI_VERSION == 9 and "#define PBR_HIP_ABI_VERSION 9" in raw and ctypes.sizeof(N.RenderDesc) == 632
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libpbr_hip.so is not built")
    lib = N.lib()
    assert lib.pbr_abi_version() == 9 and lib.pbr_render_desc_size() == 632 and lib.pbr_photometric_stereo is not None
    assert capture.CALLS["photometric_stereo"] >= 0


def test_caller_errors_come_back_without_a_device():
    """Every check runs before anything is launched: the device pointers are never dereferenced."""
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libpbr_hip.so is not built")
    lib = N.lib()
    rows = [0.1, 0.2, 0.9] * 16
    ones = [1.0] * 48
    nan, inf = float("nan"), float("inf")

    def call(targets=0x10000, weights=0x20000, shared=0, n=3, h=8, w=8, lights=rows, inten=ones, lt=N.LIGHT_POINT, size=1.0, srgb=1, k=3,
             tau=0.1, kappa=1e-4, enc=0, normal=0x30000, albedo=0x40000, conf=0x50000):
        lt_rows = None if lights is None else (ctypes.c_float * len(lights))(*lights)
        in_rows = None if inten is None else (ctypes.c_float * len(inten))(*inten)
        return lib.pbr_photometric_stereo(targets, weights, shared, n, h, w, lt_rows, in_rows, lt, size, srgb, k, tau, kappa, enc, normal, albedo, conf, None)
    for missing in ("targets", "lights", "inten", "normal", "albedo", "conf"):
        assert call(**{missing: None}) == N.ERR_NULL_MAP, missing
    assert call(n=0) == N.ERR_SHAPE and call(n=-1) == N.ERR_SHAPE and call(n=17, lights=rows + [0.0] * 3, inten=ones + [1.0] * 3) == N.ERR_SHAPE
    assert call(h=0) == N.ERR_SHAPE and call(w=0) == N.ERR_SHAPE and call(h=-2) == N.ERR_SHAPE
    assert call(h=(1 << 30) + 1) == N.ERR_SHAPE and call(h=1 << 21, w=1 << 20) == N.ERR_SHAPE          # an extent > 2^30, H * W > 2^40
    assert call(k=0) == N.ERR_SHAPE and call(k=5) == N.ERR_SHAPE and call(k=-1) == N.ERR_SHAPE
    assert call(tau=-0.01) == N.ERR_SHAPE and call(tau=1.0) == N.ERR_SHAPE and call(tau=nan) == N.ERR_SHAPE
    assert call(kappa=0.0) == N.ERR_SHAPE and call(kappa=1.0) == N.ERR_SHAPE and call(kappa=-1e-4) == N.ERR_SHAPE and call(kappa=nan) == N.ERR_SHAPE
    assert call(lt=2) == N.ERR_SHAPE and call(lt=-1) == N.ERR_SHAPE
    assert call(size=nan) == N.ERR_SHAPE and call(size=inf) == N.ERR_SHAPE
    for bad in (nan, inf, -inf):
        for at in (0, 4, 8):                                                        # an entry of the first, second and third shot
            assert call(lights=rows[:at] + [bad] + rows[at + 1:]) == N.ERR_SHAPE
            assert call(inten=ones[:at] + [bad] + ones[at + 1:]) == N.ERR_SHAPE
    assert call(inten=ones[:5] + [0.0] + ones[6:]) == N.ERR_SHAPE and call(inten=ones[:7] + [-1.0] + ones[8:]) == N.ERR_SHAPE


def test_python_argument_errors_need_no_device():
    t = torch.zeros(4, 3, 8, 8)
    light = torch.tensor([[0.1, 0.2, 0.9]] * 4)
    kw = dict(light=light, light_intensity=[1.0, 1.0, 1.0])
    ps = capture.photometric_stereo
    with pytest.raises(ValueError, match="batched"):
        ps(torch.zeros(2, 4, 3, 8, 8), **kw)
    with pytest.raises(ValueError):
        ps(torch.zeros(4, 1, 8, 8), **kw)
    with pytest.raises(ValueError):
        ps(t.numpy(), **kw)
    with pytest.raises(ValueError, match="float32"):
        ps(t.double(), **kw)
    with pytest.raises(ValueError, match="float32"):
        ps(t.half(), **kw)
    with pytest.raises(ValueError, match="at most 16"):
        ps(torch.zeros(17, 3, 8, 8), light=torch.zeros(17, 3), light_intensity=[1.0] * 3)
    for bad in (torch.ones(4, 8, 8), torch.ones(3, 1, 8, 8), torch.ones(4, 1, 8, 9), torch.ones(4, 3, 8, 8), np.ones((4, 1, 8, 8))):
        with pytest.raises(ValueError, match="weights"):
            ps(t, bad, **kw)
    with pytest.raises(ValueError, match="light_type"):
        ps(t, light_type="spot", **kw)
    for bad in (light[:3], torch.zeros(4, 2), torch.zeros(4), "north", [[0.0, 0.0, float("nan")]] * 4):
        with pytest.raises(ValueError):
            ps(t, light=bad, light_intensity=[1.0] * 3)
    for bad in ([1.0, 1.0], torch.ones(3, 3), torch.ones(5, 3), [1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, float("inf"), 1.0], [1e-60, 1.0, 1.0], None):
        with pytest.raises(ValueError):
            ps(t, light=light, light_intensity=bad)
    with pytest.raises(ValueError, match="light_size"):
        ps(t, light_size=float("nan"), **kw)
    for bad in (0, 5, -1, 2.5, True):
        with pytest.raises(ValueError, match="iterations"):
            ps(t, iterations=bad, **kw)
    for bad in (-0.1, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match="shadow_cos"):
            ps(t, shadow_cos=bad, **kw)
    for bad in (0.0, 1.0, -1e-4, float("nan"), 1e-60):
        with pytest.raises(ValueError, match="min_condition"):
            ps(t, min_condition=bad, **kw)
    with pytest.raises(ValueError, match="ROCm"):
        ps(t, **kw)                                                                 # valid arguments on the host: there is no CPU path
    with pytest.raises(ValueError, match="ROCm"):
        ps(t, torch.ones(1, 1, 8, 8, dtype=torch.bool), light_intensity=torch.ones(4, 3), light=light.tolist(), iterations=4, shadow_cos=0.0)
    with pytest.raises(ValueError, match="albedo_srgb"):
        capture.initial_material(t, albedo_srgb=False, **kw)
    with pytest.raises(ValueError, match="roughness"):
        capture.initial_material(t, roughness=1.5, **kw)
    with pytest.raises(ValueError, match="ROCm"):
        capture.initial_material(t, None, 0.6, **kw)
