"""Photometric-stereo initialisation on the device (csrc/photometric.hip, pbr_photometric_stereo; pypbr_amd.capture.photometric_stereo and
initial_material) against the oracle of its definition (tools/photometric_oracle.py, float64) on the populations
tests/test_photometric_host.py pins (tools/photometric_cases.py): 8 point lights over a 24 x 36 grid -- ragged against the kernel's tile
on both axes, the quad form -- and its 24 x 35 sibling, the pixel form.

Exact, no tolerance, on every pixel whose decisions have a margin of 1e-4 in the oracle (the share without is pinned by the host test,
at most 3 of 864): validity, the invalid pixel's normal (0, 0, 1) and confidence 0, the albedo 0 of a pixel without shots, and every
bit-for-bit statement (forms, weights=None, shared planes, NaN under a zero weight, guard bands).

Banded, on the valid pixels with that margin and c >= 0.05: normal, linear albedo and confidence.  The band is 4 x the float32-against-
float64 error of the oracle itself on the same set (hardware rsqrt, rcp, log2, exp2 at about 1 ulp each and fused multiply-adds, where
numpy float32 rounds every operation correctly), covered by the smallest of 2e-6, 1e-5, 1e-4 (24 x 36 | 24 x 35):
  gentle     4.0e-7 | 4.3e-7   -> 2e-6 | 2e-6
  shadowed   1.3e-6 | 2.1e-6   -> 1e-5 | 1e-5
  partial    4.7e-7 | 6.7e-7   -> 2e-6 | 1e-5
  rendered   4.0e-7 (host render) -> 2e-6; options: linear targets, directional lights (gentle maps) 2e-6
Measured on the MI355X, max over normal, albedo and confidence of |kernel - float64 oracle| on the banded pixels (every run prints them
before anything is asserted): gentle 5.0e-7 | 4.3e-7, shadowed 1.6e-6 | 1.3e-6, partial 5.0e-7 | 4.6e-7, rendered 4.1e-7, linear targets
4.6e-7, directional lights 2.7e-7; albedo_srgb against linear_to_srgb of the linear result 0.  End to end: median angle 0.48 degrees, stack
loss 1.8e-5 at initial_material against 2.3e-2 at flat grey, 1256 x.
Valid pixels with c < 0.05 are held to finite values, |n| = 1 within 2e-6 and an albedo in [0, 1]."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import photometric_cases as C  # noqa: E402
import photometric_oracle as O  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import capture  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = C.SIZE
L = C.N_LIGHTS
BAND = {("gentle", 36): 2e-6, ("gentle", 35): 2e-6, ("shadowed", 36): 1e-5, ("shadowed", 35): 1e-5, ("partial", 36): 2e-6, ("partial", 35): 1e-5}
EDGE, UNWRITTEN, G = -777.0, -1234.0, 256


@functools.lru_cache(maxsize=None)
def case(name, size=C.SIZE):
    return C.lambertian(name, size)


@functools.lru_cache(maxsize=None)
def oracle(name, size=C.SIZE, **kw):
    c = case(name, size)
    return O.photometric_stereo(c.targets, c.weights, c.light, c.intensity, light_size=C.LIGHT_SIZE, **kw)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(name, size=C.SIZE, **kw):
    c = case(name, size)
    weights = None if c.weights is None else dev(c.weights[:, None])
    return capture.photometric_stereo(dev(c.targets), weights, light=c.light, light_intensity=c.intensity, light_size=C.LIGHT_SIZE, **kw)


def held(what, band, got, r):
    """A launch's three results against an oracle result; the figures are printed before anything is asserted."""
    n, a, conf = (t.double().cpu().numpy() for t in got)
    conf = conf.reshape(r.confidence.shape)
    clear, invalid, banded = C.classes(r)
    low = clear & r.valid & ~banded
    e_n = np.abs(n - r.normal)[:, banded].max() if banded.any() else 0.0
    e_a = np.abs(a - r.albedo)[:, banded].max() if banded.any() else 0.0
    e_c = np.abs(conf - r.confidence)[banded].max() if banded.any() else 0.0
    print("%-30s |normal| %.2e  |albedo| %.2e  |confidence| %.2e  (band %.0e) on %d banded pixels; %d invalid with margin, %d valid with c < 0.05, %d without margin"
          % (what, e_n, e_a, e_c, band, int(banded.sum()), int(invalid.sum()), int(low.sum()), int((~clear).sum())))
    assert np.isfinite(n).all() and np.isfinite(a).all() and np.isfinite(conf).all()
    assert a.min() >= 0 and a.max() <= 1 and conf.min() >= 0
    assert np.array_equal((conf > 0)[clear], r.valid[clear]), what                   # the validity mask, exactly
    assert (n[:, invalid] == np.array([0.0, 0.0, 1.0])[:, None]).all() and (conf[invalid] == 0).all(), what
    assert max(e_n, e_a, e_c) <= band, what
    assert np.abs(np.sqrt((n * n).sum(axis=0)) - 1.0)[conf > 0].max() <= 2e-6, what
    return n, a, conf


@pytest.mark.parametrize("size", [C.SIZE, C.SIBLING])
@pytest.mark.parametrize("name", ["gentle", "shadowed", "partial"])
def test_lambertian_sets_against_the_oracle(name, size):
    before = capture.CALLS["photometric_stereo"]
    got = run(name, size)
    assert capture.CALLS["photometric_stereo"] == before + 1
    assert tuple(got[0].shape) == (3,) + size and tuple(got[1].shape) == (3,) + size and tuple(got[2].shape) == (1,) + size
    assert all(t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() for t in got)
    r = oracle(name, size)
    n, a, conf = held("%s %dx%d" % ((name,) + size), BAND[(name, size[1])], got, r)
    if name == "partial":
        seen = (case(name, size).weights != 0).sum(axis=0)
        assert (a[:, seen == 0] == 0).all() and (seen == 0).sum() >= 48              # a pixel with all weights 0: albedo exactly 0
        assert (conf[seen < 3] == 0).all()


def test_nan_targets_under_zero_weights_change_no_bit():
    c = case("partial")
    t = c.targets.copy()
    t[np.broadcast_to((c.weights == 0)[:, None], t.shape)] = np.nan
    assert np.isnan(t).mean() > 0.2
    clean = run("partial")
    dirty = capture.photometric_stereo(dev(t), dev(c.weights[:, None]), light=c.light, light_intensity=c.intensity, light_size=C.LIGHT_SIZE)
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b) and torch.isfinite(b).all()
    # masks travel as bool and uint8 too, converted as the stack steps convert them
    for kind in (torch.bool, torch.uint8):
        got = capture.photometric_stereo(dev(c.targets), dev(c.weights[:, None]).to(kind), light=c.light, light_intensity=c.intensity, light_size=C.LIGHT_SIZE)
        assert all(torch.equal(a, b) for a, b in zip(clean, got))


def test_no_weights_is_a_plane_of_ones_and_a_shared_plane_its_expansion():
    c = case("shadowed")
    t = dev(c.targets)
    kw = dict(light=c.light, light_intensity=c.intensity, light_size=C.LIGHT_SIZE)
    none = capture.photometric_stereo(t, None, **kw)
    ones = capture.photometric_stereo(t, torch.ones(L, 1, H, W, device="cuda"), **kw)
    one = capture.photometric_stereo(t, torch.ones(1, 1, H, W, device="cuda"), **kw)
    for a, b, d in zip(none, ones, one):
        assert torch.equal(a, b) and torch.equal(a, d)
    plane = torch.from_numpy(np.random.default_rng(5).uniform(0.0, 1.0, (1, 1, H, W)).astype(np.float32)).cuda()
    plane[0, 0, 3:9, 5:11] = 0.0
    shared = capture.photometric_stereo(t, plane, **kw)
    expanded = capture.photometric_stereo(t, plane.expand(L, 1, H, W).contiguous(), **kw)
    for a, b in zip(shared, expanded):
        assert torch.equal(a, b)
    assert (shared[2][0, 3:9, 5:11] == 0).all() and (shared[1][:, 3:9, 5:11] == 0).all() and (shared[2] > 0).float().mean() > 0.9
    # intensities: [3], [1,3] and [L,3] of the same values; lights as a tensor on the device
    rows = capture.photometric_stereo(t, None, light=torch.from_numpy(c.light).float().cuda(), light_intensity=torch.from_numpy(c.intensity).float().expand(L, 3),
                                      light_size=C.LIGHT_SIZE)
    assert all(torch.equal(a, b) for a, b in zip(none, rows))


@pytest.mark.parametrize("n_shots", [1, 2])
def test_fewer_than_three_shots_have_no_solution(n_shots):
    c = case("gentle")
    normal, albedo, conf = capture.photometric_stereo(dev(c.targets[:n_shots]), None, light=c.light[:n_shots], light_intensity=c.intensity,
                                                      light_size=C.LIGHT_SIZE)
    assert (conf == 0).all() and (normal[:2] == 0).all() and (normal[2] == 1).all()
    assert torch.isfinite(albedo).all() and float(albedo.max()) > 0.1               # the albedo under the flat normal, from the shots there are


def _guarded_call(case_, width, misalign=0, light_type=N.LIGHT_POINT, lights=None, weights=True):
    """pbr_photometric_stereo through the C ABI on `width` columns of a case: all three outputs inside EDGE margins with their interior
    pre-filled, `misalign` floats off 16-byte alignment.  Returns (normal, albedo, confidence) after checking the margins and that every
    element was written."""
    t = dev(case_.targets[..., :width])
    w = dev(case_.weights[..., :width]) if weights and case_.weights is not None else None
    h = t.shape[2]
    sizes = (3 * h * width, 3 * h * width, h * width)
    bufs = [torch.full((n + 2 * G + misalign,), EDGE, dtype=torch.float32, device="cuda") for n in sizes]
    views = [b[G + misalign:G + misalign + n] for b, n in zip(bufs, sizes)]
    for v in views:
        v.fill_(UNWRITTEN)
        assert (v.data_ptr() % 16 == 0) == (misalign % 4 == 0)
    rows = case_.light if lights is None else lights
    lt = (ctypes.c_float * (3 * L))(*np.asarray(rows, dtype=np.float64).reshape(-1).tolist())
    it = (ctypes.c_float * (3 * L))(*np.broadcast_to(case_.intensity, (L, 3)).reshape(-1).tolist())
    rc = N.lib().pbr_photometric_stereo(t.data_ptr(), None if w is None else w.data_ptr(), 0, L, h, width, lt, it, light_type, C.LIGHT_SIZE, 1, 3, 0.1, 1e-4, 0,
                                        views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == N.OK
    torch.cuda.synchronize()
    for buf, view in zip(bufs, views):
        lo = G + misalign
        assert (buf[:lo] == EDGE).all() and (buf[lo + view.numel():] == EDGE).all()              # canaries in front and behind
        assert not (view == UNWRITTEN).any() and not (view == EDGE).any() and torch.isfinite(view).all()       # every element written
    return views[0].view(3, h, width).clone(), views[1].view(3, h, width).clone(), views[2].view(1, h, width).clone()


@pytest.mark.parametrize("name", ["shadowed", "partial"])
def test_guard_bands_and_the_two_forms_give_the_same_bits(name):
    c = case(name)
    quad = _guarded_call(c, 36)                                                     # the quad form
    held("guarded " + name, BAND[(name, 36)], quad, oracle(name))
    via_python = run(name)
    assert all(torch.equal(a, b) for a, b in zip(quad, via_python))
    pixel = _guarded_call(c, 36, misalign=1)                                        # the same launch 4 bytes off alignment: the pixel form
    assert all(torch.equal(a, b) for a, b in zip(quad, pixel))
    # a width 4 does not divide, on the common pixels: directional lights, whose geometry does not depend on the grid's width
    dirs = c.light / np.linalg.norm(c.light, axis=1, keepdims=True)
    wide = _guarded_call(c, 36, light_type=N.LIGHT_DIRECTIONAL, lights=dirs)
    narrow = _guarded_call(c, 35, light_type=N.LIGHT_DIRECTIONAL, lights=dirs)
    assert all(torch.equal(a[..., :35], b) for a, b in zip(wide, narrow))


def test_two_calls_give_the_same_bits():
    for name in ("gentle", "shadowed", "partial"):
        a, b = run(name, albedo_srgb=True), run(name, albedo_srgb=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_albedo_srgb_is_the_encoded_linear_result():
    lin = run("shadowed")
    enc = run("shadowed", albedo_srgb=True)
    assert torch.equal(lin[0], enc[0]) and torch.equal(lin[2], enc[2])
    err = float((enc[1] - F.linear_to_srgb(lin[1])).abs().max())
    print("albedo_srgb against linear_to_srgb of the linear result: %.2e (band 2e-6)" % err)
    assert err <= 2e-6 and not torch.equal(lin[1], enc[1])


def test_linear_targets_against_the_oracle():
    c = case("gentle")
    lin = O.srgb_to_linear(c.targets.astype(np.float64)).astype(np.float32)
    got = capture.photometric_stereo(dev(lin), None, light=c.light, light_intensity=c.intensity, light_size=C.LIGHT_SIZE, targets_srgb=False)
    r = O.photometric_stereo(lin, None, c.light, c.intensity, light_size=C.LIGHT_SIZE, targets_srgb=False)
    held("gentle, linear targets", 2e-6, got, r)


def test_directional_lights_and_other_options_against_the_oracle():
    c = case("gentle")
    dirs = 2.5 * c.light                                                            # not unit: the entry point normalises
    unit = c.light / np.linalg.norm(c.light, axis=1, keepdims=True)
    lin = (np.maximum((unit[:, :, None, None] * c.normal[None]).sum(axis=1), 0)[:, None] * c.albedo[None] / np.pi * 2.0)
    targets = O.linear_to_srgb(lin).astype(np.float32)
    inten = np.full(3, 2.0)
    for kw in (dict(), dict(iterations=1), dict(iterations=4, shadow_cos=0.3, min_condition=0.5)):
        got = capture.photometric_stereo(dev(targets), None, light=dirs, light_intensity=inten, light_type="directional", **kw)
        r = O.photometric_stereo(targets, None, dirs, inten, light_type="directional", **kw)
        held("gentle, directional %s" % (kw,), 2e-6, got, r)
    assert not r.valid.all() and r.valid.mean() > 0.5                               # min_condition 0.5 rejects a part (4 % of the pixels)


def test_end_to_end_initial_material_starts_the_fit_close():
    """The gentle maps rendered as a rough dielectric on the device: the stack loss at initial_material is at least 100 x below the loss at
    a flat normal with grey albedo (float64 with the reference model: 1256 x), the normals are within 1 degree in the median (0.48)."""
    c = case("gentle")
    known = [dev(c.albedo.astype(np.float32)), dev(c.normal.astype(np.float32)), torch.full((1, H, W), C.ROUGHNESS, device="cuda"), torch.zeros(1, H, W, device="cuda")]
    kw = dict(view_dir=[0.0, 0.0, 1.0], light=torch.from_numpy(c.light).float(), light_intensity=c.intensity.tolist(), light_type="point",
              light_size=C.LIGHT_SIZE)
    targets = F.cook_torrance_stack(*known, albedo_is_srgb=False, **kw)             # [L,3,H,W], sRGB
    assert tuple(targets.shape) == (L, 3, H, W) and float(targets.max()) < 1.0
    r = O.photometric_stereo(targets.cpu().numpy(), None, c.light, c.intensity, light_size=C.LIGHT_SIZE)
    before = capture.CALLS["photometric_stereo"]
    got = capture.photometric_stereo(targets, None, light=c.light, light_intensity=c.intensity, light_size=C.LIGHT_SIZE)
    material = capture.initial_material(targets, None, C.ROUGHNESS, light=c.light, light_intensity=c.intensity, light_size=C.LIGHT_SIZE)
    assert capture.CALLS["photometric_stereo"] == before + 2                        # one launch per call
    held("rendered", 2e-6, got, r)
    from pypbr_amd.materials import BasecolorMetallicMaterial
    assert isinstance(material, BasecolorMetallicMaterial) and material.albedo_is_srgb
    assert torch.equal(material.normal, got[0]) and float((material.albedo - F.linear_to_srgb(got[1])).abs().max()) <= 2e-6
    assert float(material.roughness.min()) == float(material.roughness.max()) == pytest.approx(C.ROUGHNESS) and not material.metallic.any()
    cos = (got[0].double().cpu().numpy() * c.normal).sum(axis=0)
    median = float(np.median(np.degrees(np.arccos(np.clip(cos, -1, 1)))))

    def loss(albedo, normal):
        maps = [albedo.clone().requires_grad_(True), normal.clone().requires_grad_(True), known[2], known[3]]
        value = F.rendering_loss_mse_stack(*maps, targets=targets, **kw)
        value.backward()                                                            # ready for a fit: gradients flow into the maps
        assert maps[0].grad is not None and torch.isfinite(maps[0].grad).all() and torch.isfinite(maps[1].grad).all()
        return float(value)
    flat = torch.zeros(3, H, W, device="cuda")
    flat[2] = 1.0
    at_start, at_flat = loss(material.albedo, material.normal), loss(torch.full((3, H, W), 0.5, device="cuda"), flat)
    print("rendered: median angle %.3f degrees; stack loss %.3e at initial_material, %.3e at flat grey: %.0f x" % (median, at_start, at_flat, at_flat / at_start))
    assert median < 1.0
    assert at_flat >= 100 * at_start
