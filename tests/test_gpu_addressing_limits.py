"""Kernels at their 32-bit addressing limits.

Scalar plane addressing (ct_kernel.hpp: KArgs::sbase, plane_at) adds a per-lane 32-BIT byte offset to a wave-uniform 64-bit plane base; the
host decides, per launch family, whether every lane offset fits.  Everything else indexes with 64 bits per lane.  Each test here renders at a
shape where one of those offsets crosses a 32-bit boundary, and checks
  * windows at the FAR end (last material / plane, last rows, last columns) and the first window against a float64 reference,
  * where a second form of the same launch exists, bit-equality with it over the whole result: per-call `tuning={"scalar_base": 0}`
    (per-lane 64-bit addresses, same arithmetic) or the wrap-around form of tiled maps (PBR_TUNE_TILE_REPEAT = 0, as test_gpu_round6.py),
  * non-vacuity: the reference at the place a wrapped offset would reach differs from the true reference by more than the tolerance
    (seeded, non-periodic data), so a wrap could not pass the window check.

test -> the offset that crosses a 32-bit boundary
  thin_band_of_a_wide_tiled_image ........... result lane offset sy*out_W up to 2^31 elements (fp32: 2^33 bytes); 2^32 bytes = 8192 rows
  thin_band_fp16_result ..................... result lane offset 20000*131072 = 2.6e9 > 2^31 elements (the int product overflows too)
  thin_band_texel_offsets_beyond_2_to_30 .... texel lane offset sy*map_w up to 1.0743e9 > 2^30 elements (2^32 bytes of fp32)
  thin_band_that_keeps_scalar_bases ......... map_h*out_W = 1.0732e9 < 2^30: scalar bases stay on, offsets pass 2^31 bytes
  fused_blend_thin_band ..................... as thin_band_of_a_wide_tiled_image, both materials and the mask
  folded_backward_of_a_thin_band ............ upstream lane offset 12000*131072 > 2^30 elements (2^32 bytes of fp32)
  scalar_bases_at_their_limit_* ............. 32752*32768 = 1.0732e9 px: fp32 offsets to 2^32 - 2 MiB bytes (past 2^31)
  batch_past_2_to_31_elements_* ............. material 11 of 12 x 8192^2 starts at 2.2e9 elements (batched planes: 64-bit lanes)
  map_ops_past_2_to_31_elements ............. 3 x 32768 x 32768 = 3.2e9 elements in one tensor

The thin-band tests pin the fix of fill_repeat_args / fill_repeat_backward (ct_tiled.hip, ct_repeat_backward.hip): a band thinner than one
period walks source rows anywhere in [0, map_h), so the scalar-base rule must use map_h * out_W and map_h * map_w, not the band's rows.
Every test guards its device memory with torch.cuda.mem_get_info() and skips, saying what it needs, on a smaller device."""

import gc

import numpy as np
import pytest
import torch

import blend_oracle as BO
import c_oracle as C
import torch_oracle as O
from test_gpu_parity import TOL, parity_report

pytestmark = pytest.mark.gpu

GiB = 1 << 30
SET = "addressing limits"
POINT = dict(view_dir=[0.05, 0.1, 0.9], light_type="point", light_size=1.5)
DIRECTIONAL = dict(view_dir=[0.05, 0.1, 0.9], light_type="directional", light_size=None)
POINT_LIGHTS = ([[0.1, 0.1, 1.0], [-0.4, 0.2, 0.7], [0.3, -0.3, 0.9]], [[1.0, 0.9, 0.8], [0.4, 0.5, 0.6], [0.3, 0.3, 0.3]])
DIR_LIGHTS = ([[0.3, -0.2, 1.0], [0.1, 0.4, 0.8], [-0.2, 0.1, 1.0]], POINT_LIGHTS[1])


@pytest.fixture(autouse=True)
def _release_device_memory(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\n[{request.node.name}] peak device memory {torch.cuda.max_memory_allocated() / GiB:.1f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


def _need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GiB:
        pytest.skip(f"needs {gib} GiB of free device memory, {free / GiB:.1f} GiB free")


def _kw(light_type, lights=1):
    L, I = POINT_LIGHTS if light_type == "point" else DIR_LIGHTS
    base = POINT if light_type == "point" else DIRECTIONAL
    return dict(base, light=L[:lights] if lights > 1 else L[0], light_intensity=I[:lights] if lights > 1 else I[0])


def _maps(h, w, seed, dtype=torch.float32, normal=True, B=None):
    """Seeded, non-periodic maps made on the device (no host copy of tens of GiB): roughness in [0.3, 1] (criterion (i) holds there),
    signed z-dominant normals that are not unit length (the kernels normalise)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lead = () if B is None else (B,)
    a = torch.rand(*lead, 3, h, w, device="cuda", generator=g, dtype=dtype)
    n = None
    if normal:
        n = torch.rand(*lead, 3, h, w, device="cuda", generator=g, dtype=dtype)
        n[..., :2, :, :] -= 0.5
        n[..., 2, :, :] += 0.5
    r = torch.rand(*lead, 1, h, w, device="cuda", generator=g, dtype=dtype).mul_(0.7).add_(0.3)
    m = torch.rand(*lead, 1, h, w, device="cuda", generator=g, dtype=dtype)
    return [a, n, r, m]


def _knob_tile_repeat(value):
    from pypbr_amd import _native as N
    N.lib().pbr_set_tuning(N.TUNE_TILE_REPEAT, value)


def _wrap_around_form(*args, **kw):
    from pypbr_amd import functional as F
    try:
        _knob_tile_repeat(0)
        return F.cook_torrance(*args, **kw)
    finally:
        _knob_tile_repeat(-1)


def _tiled_rows(maps, y0, rows, tile):
    """The rows [y0, y0 + rows) of the tiled maps, materialised horizontally on the host: [C, rows, nx * map_w] float32 (exact for fp16)."""
    ny, nx = tile
    mh = maps[0].shape[-2]
    sy = torch.tensor([(y0 + i) % mh for i in range(rows)], device=maps[0].device)
    return [None if t is None else t.index_select(-2, sy).float().cpu().repeat(1, 1, nx) for t in maps]


def _lights(kw):
    return np.asarray(kw["light"], np.float64).reshape(-1, 3), np.asarray(kw["light_intensity"], np.float64).reshape(-1, 3)


def _ref64(crop, kw, y0, H_total):
    L, I = _lights(kw)
    return C.render(*[None if t is None else t.numpy() for t in crop], None, view=kw["view_dir"], lights=L, intensities=I,
                    light_type=kw["light_type"], light_size=kw["light_size"], y_offset=y0, H_total=H_total, dtype=np.float64)


def _ref32(crop, kw, y0, H_total):
    L, I = _lights(kw)
    okw = dict(view=torch.tensor(kw["view_dir"]), light_type=kw["light_type"], light_size=kw["light_size"], y_offset=y0, H_total=H_total)
    if L.shape[0] > 1:
        return O.cook_torrance_multi(*crop, None, lights=torch.tensor(L, dtype=torch.float32), intensities=torch.tensor(I, dtype=torch.float32),
                                     **okw).numpy()
    return O.cook_torrance(*crop, None, light=torch.tensor(L[0], dtype=torch.float32), intensity=torch.tensor(I[0], dtype=torch.float32),
                           **okw).numpy()


def _parity(got, crop, kw, y0, H_total, what):
    """The suite's parity criterion (test_gpu_parity.py) on a window: float64 C oracle and the ATen restatement in fp32."""
    ref64 = _ref64(crop, kw, y0, H_total)
    parity_report(got.float().cpu().numpy(), _ref32(crop, kw, y0, H_total), ref64, crop[2].numpy(), what=(SET,) + tuple(what))
    return ref64


def _distinct(true_ref, wrapped_ref, tol, what):
    """Non-vacuity: what a wrapped offset would reach is not what the window must hold."""
    diff = float(np.abs(np.asarray(true_ref, np.float64) - np.asarray(wrapped_ref, np.float64)).max())
    assert diff > tol, (what, "the reference at the wrapped location equals the true one within the tolerance: the check would be vacuous", diff)


def _equal_to_host(dev, host, what):
    """Bit-equality of a device tensor with a host copy, a slice at a time (no second device copy of tens of GiB)."""
    d, h = dev.reshape(-1), host.reshape(-1)
    assert d.numel() == h.numel(), what
    step = 1 << 28
    for i in range(0, d.numel(), step):
        assert torch.equal(d[i:i + step].cpu(), h[i:i + step]), (what, "elements from", i)


# ---------------------------------------------------------------- (a) thin bands of a tiled image: the repeat-inner walk's scalar-base rule
@pytest.mark.parametrize("light_type,lights", [("point", 1), ("point", 3), ("directional", 1), ("directional", 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("y0", [12000, 16380, 8190])
def test_thin_band_of_a_wide_tiled_image(y0, dtype, light_type, lights):
    """16384 x 256 maps under tile (1, 512): a 16384 x 131072 image.  A 4-row band is thinner than the period, so the walk addresses source
    rows sy = y0 .. y0 + 3 and its lane offset is sy * 131072 + x -- past 2^30 elements (2^32 bytes of fp32) from row 8192 on.  (8190, 4)
    straddles that boundary.  Bit-equal to the wrap-around form, and the band and the image's first rows within the parity criterion."""
    from pypbr_amd import functional as F
    _need(2)
    mh, mw, tile, rows = 16384, 256, (1, 512), 4
    out_W, H_total = tile[1] * mw, tile[0] * mh
    maps = _maps(mh, mw, 1000 + y0 + lights, dtype)
    kw = _kw(light_type, lights)
    plan = F.plan_cook_torrance(*maps, tile=tile, y_offset=y0, rows=rows, **kw)
    assert plan.kernel_name.startswith("ctr_"), plan.kernel_name
    got = plan.launch().clone()
    assert got.shape == (1, 3, rows, out_W) or got.shape == (3, rows, out_W)
    got = got.reshape(3, rows, out_W)
    assert torch.equal(got, _wrap_around_form(*maps, tile=tile, y_offset=y0, rows=rows, **kw).reshape(3, rows, out_W))
    ref = _parity(got, _tiled_rows(maps, y0, rows, tile), kw, y0, H_total, ("thin band", y0, str(dtype), light_type, lights))
    first = F.cook_torrance(*maps, tile=tile, y_offset=0, rows=rows, **kw).reshape(3, rows, out_W)
    _parity(first, _tiled_rows(maps, 0, rows, tile), kw, 0, H_total, ("thin band, first rows", str(dtype), light_type, lights))
    # a wrapped fp32 store lands 2^32 bytes = 2^30 / out_W = 8192 rows earlier in the image
    shift = (1 << 30) // out_W
    wrapped = [y for y in range(y0, y0 + rows) if y >= shift]
    assert wrapped, "the band must cross 2^30 elements"
    k = wrapped[0] - y0
    _distinct(ref[:, k:], _ref64(_tiled_rows(maps, wrapped[0] - shift, len(wrapped), tile), kw, wrapped[0] - shift, H_total), TOL, "thin band")


def test_thin_band_fp16_result():
    """fp16 result: 32768 x 128 maps under tile (1, 1024), band (20000, 4).  sy * out_W = 2.6e9 > 2^31 elements: past the 32-bit byte offset of
    fp16 (2^31 elements) and past the int product.  Bit-equal to the wrap-around form; within fp16 rounding (2^-11 in [0, 1]) of float64."""
    from pypbr_amd import functional as F
    _need(2)
    mh, mw, tile, y0, rows = 32768, 128, (1, 1024), 20000, 4
    out_W = tile[1] * mw
    maps = _maps(mh, mw, 77)
    kw = dict(_kw("point"), out_dtype=torch.float16)
    got = F.cook_torrance(*maps, tile=tile, y_offset=y0, rows=rows, **kw).reshape(3, rows, out_W)
    assert got.dtype == torch.float16
    assert torch.equal(got, _wrap_around_form(*maps, tile=tile, y_offset=y0, rows=rows, **kw).reshape(3, rows, out_W))
    ref_kw = _kw("point")
    ref = _ref64(_tiled_rows(maps, y0, rows, tile), ref_kw, y0, mh)
    tol = 2.0 ** -11
    assert np.abs(got.double().cpu().numpy() - ref).max() <= tol
    first = F.cook_torrance(*maps, tile=tile, y_offset=0, rows=rows, **kw).reshape(3, rows, out_W)
    assert np.abs(first.double().cpu().numpy() - _ref64(_tiled_rows(maps, 0, rows, tile), ref_kw, 0, mh)).max() <= tol
    shift = (1 << 31) // out_W                                       # a wrapped fp16 store: 2^32 bytes = 2^31 elements = 16384 rows earlier
    _distinct(ref, _ref64(_tiled_rows(maps, y0 - shift, rows, tile), ref_kw, y0 - shift, mh), tol, "fp16 thin band")


def test_thin_band_texel_offsets_beyond_2_to_30():
    """Texel offsets: fp32 maps 32768 x 32784 (1.0743e9 texels per plane, above 2^30) under tile (2, 1), band (32704, 64).  The walk loads
    source rows 32704 .. 32767 at sy * 32784 + x: past 2^30 elements (2^32 bytes) from row 32752 on -- a band's height times the map's width
    is what the launch was checking.  About 34 GiB of maps."""
    from pypbr_amd import functional as F
    _need(40)
    mh, mw, tile, y0, rows = 32768, 32784, (2, 1), 32704, 64
    maps = _maps(mh, mw, 91)
    kw = _kw("point")
    plan = F.plan_cook_torrance(*maps, tile=tile, y_offset=y0, rows=rows, **kw)
    assert plan.kernel_name.startswith("ctr_"), plan.kernel_name
    got = plan.launch().clone().reshape(3, rows, mw)
    del plan
    assert torch.equal(got, _wrap_around_form(*maps, tile=tile, y_offset=y0, rows=rows, **kw).reshape(3, rows, mw))
    ref = _parity(got, _tiled_rows(maps, y0, rows, tile), kw, y0, 2 * mh, ("texel facet", y0))
    first = F.cook_torrance(*maps, tile=tile, y_offset=0, rows=4, **kw).reshape(3, 4, mw)
    _parity(first, _tiled_rows(maps, 0, 4, tile), kw, 0, 2 * mh, ("texel facet, first rows",))
    # non-vacuity: the last 8 rows' texels all lie past 2^30 elements; a wrapped load reads the texel 2^30 elements earlier
    k0 = rows - 8
    assert (y0 + k0) * mw >= 1 << 30
    e = (torch.arange(y0 + k0, y0 + rows, device="cuda")[:, None] * mw + torch.arange(mw, device="cuda")[None, :]) - (1 << 30)
    wrapped = [t.reshape(t.shape[0], -1)[:, e].float().cpu() for t in maps]
    _distinct(ref[:, k0:], _ref64(wrapped, kw, y0 + k0, 2 * mh), TOL, "texel facet")


def test_thin_band_that_keeps_scalar_bases():
    """The bracket: 16376 x 256 maps under tile (1, 256), band (16372, 4).  map_h * out_W = 1.0732e9 < 2^30, so the walk keeps scalar plane
    addresses; its lane offsets pass 2^31 bytes (a signed 32-bit offset would wrap 8192 rows back).  Default, scalar_base = 0 and
    scalar_base = 2 bit-equal, and the band within the parity criterion.  Nothing reports whether a launch took scalar bases, so this test
    catches a wrong answer on either side of the rule, not an over-conservative rule that turns them off here (a speed matter only)."""
    from pypbr_amd import functional as F
    _need(2)
    mh, mw, tile, y0, rows = 16376, 256, (1, 256), 16372, 4
    out_W = tile[1] * mw
    assert mh * out_W < 1 << 30
    maps = _maps(mh, mw, 123)
    kw = _kw("point")
    outs = [F.cook_torrance(*maps, tile=tile, y_offset=y0, rows=rows, tuning=t, **kw).reshape(3, rows, out_W)
            for t in (None, {"scalar_base": 0}, {"scalar_base": 2})]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    ref = _parity(outs[0], _tiled_rows(maps, y0, rows, tile), kw, y0, mh, ("bracket", y0))
    shift = (1 << 29) // out_W                                       # 2^31 bytes of fp32
    _distinct(ref, _ref64(_tiled_rows(maps, y0 - shift, rows, tile), kw, y0 - shift, mh), TOL, "bracket")


# ---------------------------------------------------------------- (b) the fused blend over tiled maps, thin band
def _blend_ref64(m1, m2, mask, y0, rows, tile, kw):
    """float64: blend_with_mask on the band's rows (materialised horizontally), the blended normal re-decoded, the BRDF."""
    names = ("albedo", "normal", "roughness", "metallic")
    c1, c2 = _tiled_rows(m1, y0, rows, tile), _tiled_rows(m2, y0, rows, tile)
    cm = _tiled_rows([mask], y0, rows, tile)[0]
    bl = BO.blend_materials({k: v.double() for k, v in zip(names, c1)}, {k: v.double() for k, v in zip(names, c2)}, cm.double())
    L, I = _lights(kw)
    return O.cook_torrance(bl["albedo"], bl["normal"], bl["roughness"], bl["metallic"], view=torch.tensor(kw["view_dir"], dtype=torch.float64),
                           light=torch.tensor(L[0]), intensity=torch.tensor(I[0]), light_type=kw["light_type"], light_size=kw["light_size"],
                           y_offset=y0, H_total=tile[0] * m1[0].shape[-2]).numpy()


@pytest.mark.parametrize("light_type", ["point", "directional"])
@pytest.mark.parametrize("y0", [12000, 8190])
def test_fused_blend_thin_band(y0, light_type):
    """cook_torrance(blend=..., tile=(1, 512)) on a 4-row band of the 16384 x 131072 image: the blend walk (cook_torrance_repeat_blend_kernel)
    takes fill_repeat_args' rule.  Bit-equal to the wrap-around form, within 1e-5 of float64 blend + BRDF on the band's rows."""
    from pypbr_amd import functional as F
    _need(2)
    mh, mw, tile, rows = 16384, 256, (1, 512), 4
    out_W = tile[1] * mw
    m1, m2 = _maps(mh, mw, 500 + y0), _maps(mh, mw, 600 + y0)
    mask = torch.rand(1, mh, mw, device="cuda", generator=torch.Generator(device="cuda").manual_seed(700 + y0))
    kw = _kw(light_type)
    second = (m2[0], m2[1], m2[2], m2[3], None, mask)
    got = F.cook_torrance(*m1, blend=second, tile=tile, y_offset=y0, rows=rows, **kw).reshape(3, rows, out_W)
    assert torch.equal(got, _wrap_around_form(*m1, blend=second, tile=tile, y_offset=y0, rows=rows, **kw).reshape(3, rows, out_W))
    ref = _blend_ref64(m1, m2, mask, y0, rows, tile, kw)
    assert np.abs(got.double().cpu().numpy() - ref).max() <= TOL
    first = F.cook_torrance(*m1, blend=second, tile=tile, y_offset=0, rows=rows, **kw).reshape(3, rows, out_W)
    assert np.abs(first.double().cpu().numpy() - _blend_ref64(m1, m2, mask, 0, rows, tile, kw)).max() <= TOL
    shift = (1 << 30) // out_W
    w0 = max(y0, shift)
    _distinct(ref[:, w0 - y0:], _blend_ref64(m1, m2, mask, w0 - shift, y0 + rows - w0, tile, kw), TOL, "fused blend thin band")


# ---------------------------------------------------------------- (c) the folded backward of a thin band
def _folded_grad_ref(maps, gout, y0, rows, tile, kw):
    """float64 autograd through the repeat of the band's rows: per texel, the sum over its nx repeats and the sum of their magnitudes."""
    nx = tile[1]
    crop = [None if t is None else t.double().requires_grad_() for t in _tiled_rows(maps, y0, rows, tile)]
    L, I = _lights(kw)
    ref = O.cook_torrance(*crop, None, view=torch.tensor(kw["view_dir"], dtype=torch.float64), light=torch.tensor(L[0]), intensity=torch.tensor(I[0]),
                          light_type=kw["light_type"], light_size=kw["light_size"], y_offset=y0, H_total=tile[0] * maps[0].shape[-2])
    (ref * gout.double()).sum().backward()
    mw = maps[0].shape[-1]
    folded = [None if t is None else t.grad.reshape(t.shape[0], rows, nx, mw) for t in crop]
    return [None if g is None else g.sum(2) for g in folded], [None if g is None else g.abs().sum(2) for g in folded]


@pytest.mark.parametrize("light_type", ["point", "directional"])
def test_folded_backward_of_a_thin_band(light_type):
    """MaterialBase.tile under autograd on a 4-row band (12000, 4) of the 16384 x 131072 image: the folded backward reads its upstream gradient at
    sy * 131072 + x, past 2^30 elements (2^32 bytes).  Map-sized gradients against float64 autograd through the repeat; exactly zero in the
    texel rows the band does not touch.  Bound per texel: each of the 512 repeats within the per-pixel criterion of test_gpu_backward.py,
    2e-5 (1 + |g_k|), plus fp32 rounding of the 512-term sum, 512 * 2^-24 * sum|g_k|."""
    from pypbr_amd import functional as F
    _need(2)
    mh, mw, tile, y0, rows = 16384, 256, (1, 512), 12000, 4
    nx, out_W = tile[1], tile[1] * mw
    maps = _maps(mh, mw, 31)
    kw = _kw(light_type)
    gout = torch.rand(3, rows, out_W, generator=torch.Generator().manual_seed(32)) - 0.4
    leaves = [t.clone().requires_grad_() for t in maps]
    out = F.cook_torrance(*leaves, tile=tile, y_offset=y0, rows=rows, **kw)
    (out.reshape(3, rows, out_W) * gout.cuda()).sum().backward()
    want, mag = _folded_grad_ref(maps, gout, y0, rows, tile, kw)
    for name, leaf, g64, s in zip(("albedo", "normal", "roughness", "metallic"), leaves, want, mag):
        g = leaf.grad
        assert g.shape == leaf.shape, name
        band = g[:, y0:y0 + rows].double().cpu()
        bound = 2e-5 * (nx + s) + nx * 2.0 ** -24 * s
        assert bool(((band - g64).abs() <= bound).all()), (name, float((band - g64).abs().max()))
        assert not bool(g[:, :y0].any()) and not bool(g[:, y0 + rows:].any()), (name, "gradient outside the band's texel rows")
    # non-vacuity: the gradient the texels 2^32 bytes (8192 image rows) earlier would get from the same upstream values
    shift = (1 << 30) // out_W
    other, _ = _folded_grad_ref(maps, gout, y0 - shift, rows, tile, kw)
    _distinct(want[0].numpy(), other[0].numpy(), float((2e-5 * (nx + mag[0]) + nx * 2.0 ** -24 * mag[0]).max()), "folded backward")


# ---------------------------------------------------------------- (d) scalar bases at their limit: one material of 32752 x 32768 (< 2^30 px)
LH, LW = 32752, 32768
SIGNED_SHIFT = (1 << 29) // LW          # 2^31 bytes of fp32 = 16384 rows: where a signed 32-bit byte offset would wrap to


def _window_rows():
    return (0, LH - 4)


def test_scalar_bases_at_their_limit_forward_fp32():
    """Forward, fp32 maps: one plane holds 1.0732e9 px, just under 2^30, so the launch keeps scalar plane addresses and its 32-bit lane
    offsets reach 2^32 - 2 MiB bytes.  The whole result bit-equal to scalar_base = 0; first and last rows (all columns) within the parity
    criterion.  Measured peak 59 GiB."""
    from pypbr_amd import functional as F
    _need(66)
    maps = _maps(LH, LW, 41)
    kw = _kw("point")
    got = F.cook_torrance(*maps, **kw)
    per_lane = F.cook_torrance(*maps, tuning={"scalar_base": 0}, **kw)
    assert torch.equal(got, per_lane)
    del per_lane
    got = got.reshape(3, LH, LW)
    for y0 in _window_rows():
        crop = [t[:, y0:y0 + 4].float().cpu() for t in maps]
        ref = _parity(got[:, y0:y0 + 4], crop, kw, y0, LH, ("limit forward", y0))
    crop = [t[:, LH - 4 - SIGNED_SHIFT:LH - SIGNED_SHIFT].float().cpu() for t in maps]
    _distinct(ref, _ref64(crop, kw, LH - 4 - SIGNED_SHIFT, LH), TOL, "limit forward")


def _grads_at_limit(maps, kw, gout, tuning):
    from pypbr_amd import functional as F
    for t in maps:
        if t is not None:
            t.grad = None
    out = F.cook_torrance(*maps, tuning=tuning, **kw)
    out.backward(gout.reshape(out.shape))
    del out
    return [None if t is None else t.grad for t in maps]


def _backward_window_ref(maps, gout, y0, kw):
    crop = [None if t is None else t[:, y0:y0 + 4].double().cpu().requires_grad_() for t in maps]
    L, I = _lights(kw)
    ref = O.cook_torrance(*crop, None, view=torch.tensor(kw["view_dir"], dtype=torch.float64), light=torch.tensor(L[0]), intensity=torch.tensor(I[0]),
                          light_type=kw["light_type"], light_size=kw["light_size"], y_offset=y0, H_total=LH)
    (ref * gout.double()).sum().backward()
    return [None if t is None else t.grad for t in crop]


@pytest.mark.parametrize("dtype,normal,second", [(torch.float16, True, {"bwd_run": 0}), (torch.float32, False, {"scalar_base": 0})],
                         ids=["f16-streamed", "f32-one-tile"])
def test_scalar_bases_at_their_limit_backward(dtype, normal, second):
    """Backward of one 32752 x 32768 material; the fp32 upstream gradient's lane offsets reach 2^32 - 2 MiB bytes.
    fp16 maps: the streamed kernel, which always addresses through scalar bases (ct_backward_stream.hpp) and is only chosen for planes below 2^30 px
    (stream_run); its second form is the one-tile kernels (bwd_run = 0), whose scalar bases follow fill_args.  fp32 maps: the one-tile kernel
    (without a normal map, to keep the footprint down), second form scalar_base = 0.  Every gradient plane bit-equal to the second form; the
    first and last rows against float64 autograd (test_gpu_backward.py's criteria: fp32 2e-5 (1 + |g|), fp16 storage 1e-3 (1e-3 + |g|)).
    Measured peaks: 68 GiB (fp16), 76 GiB (fp32)."""
    _need(84 if dtype == torch.float32 else 76)
    maps = [None if t is None else t.requires_grad_() for t in _maps(LH, LW, 43, dtype, normal=normal)]
    kw = _kw("point")
    gout = torch.rand(3, LH, LW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(44)).sub_(0.4)
    host = [None if g is None else g.cpu() for g in _grads_at_limit(maps, kw, gout, None)]
    per_lane = _grads_at_limit(maps, kw, gout, second)
    names = ("albedo", "normal", "roughness", "metallic")
    for name, g, h in zip(names, per_lane, host):
        if g is not None:
            _equal_to_host(g, h, name)
    del per_lane
    for t in maps:
        if t is not None:
            t.grad = None

    def close(got, want):
        if dtype == torch.float16:
            return (got - want).abs() <= 1e-3 * (1e-3 + want.abs()) + 2e-5 * (1 + want.abs())
        return (got - want).abs() <= 2e-5 * (1 + want.abs())
    maps_d = [None if t is None else t.detach() for t in maps]
    for y0 in _window_rows():
        want = _backward_window_ref(maps_d, gout[:, y0:y0 + 4].cpu(), y0, kw)
        for name, h, w in zip(names, host, want):
            if h is not None:
                assert bool(close(h[:, y0:y0 + 4].double(), w).all()), (name, y0, float((h[:, y0:y0 + 4].double() - w).abs().max()))
    # non-vacuity: the upstream values 2^31 bytes earlier (a signed 32-bit offset's wrap) give the last rows other gradients
    y0 = LH - 4
    wrong = _backward_window_ref(maps_d, gout[:, y0 - SIGNED_SHIFT:y0 + 4 - SIGNED_SHIFT].cpu(), y0, kw)
    _distinct(want[0].numpy(), wrong[0].numpy(), float((1e-3 * (1e-3 + want[0].abs()) + 2e-5 * (1 + want[0].abs())).max()), "limit backward")


def test_scalar_bases_at_their_limit_mse_step():
    """The rendering-loss step (pbr_cook_torrance_mse_step: loss and gradients from one kernel) on one 32752 x 32768 material, fp32 maps without
    a normal map: the target's lane offsets reach 2^32 - 2 MiB bytes.  Loss and gradients bit-equal to scalar_base = 0; the loss within 1e-5
    (relative) of the float64 mean over the library's own forward result (a consistency check of the kernel's reduction; the gradient windows
    are the independent float64 check); the first and last rows' gradients against float64 autograd.  Measured peak 52 GiB."""
    from pypbr_amd import functional as F
    _need(60)
    maps = [None if t is None else t.requires_grad_() for t in _maps(LH, LW, 47, normal=False)]
    kw = _kw("point")
    target = torch.rand(3, LH, LW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(48))

    def step(tuning):
        for t in maps:
            if t is not None:
                t.grad = None
        loss = F.rendering_loss_mse(*maps, target=target, tuning=tuning, **kw)
        loss.backward()
        return loss.detach().clone(), [None if t is None else t.grad for t in maps]
    loss, grads = step(None)
    host = [None if g is None else g.cpu() for g in grads]
    del grads
    loss0, grads0 = step({"scalar_base": 0})
    assert torch.equal(loss, loss0)
    for name, g, h in zip(("albedo", "normal", "roughness", "metallic"), grads0, host):
        if g is not None:
            _equal_to_host(g, h, name)
    del grads0
    for t in maps:
        if t is not None:
            t.grad = None
    maps_d = [None if t is None else t.detach() for t in maps]
    with torch.no_grad():
        out = F.cook_torrance(*maps_d, **kw).reshape(3, LH, LW)
        n = out.numel()
        loss64 = sum(float(((out[c, y:y + 4096].double() - target[c, y:y + 4096].double()) ** 2).sum()) for c in range(3) for y in range(0, LH, 4096)) / n
        del out
    assert abs(float(loss.detach()) - loss64) <= 1e-5 * loss64, (float(loss.detach()), loss64)
    L, I = _lights(kw)
    for y0 in _window_rows():
        crop = [None if t is None else t[:, y0:y0 + 4].double().cpu().requires_grad_() for t in maps_d]
        ref = O.cook_torrance(*crop, None, view=torch.tensor(kw["view_dir"], dtype=torch.float64), light=torch.tensor(L[0]), intensity=torch.tensor(I[0]),
                              light_type="point", light_size=kw["light_size"], y_offset=y0, H_total=LH)
        ((ref - target[:, y0:y0 + 4].double().cpu()) ** 2).sum().div(n).backward()
        for name, h, c in zip(("albedo", "normal", "roughness", "metallic"), host, crop):
            if h is None:
                continue
            want, got = c.grad, h[:, y0:y0 + 4].double()
            assert bool(((got - want).abs() <= 2e-5 * (want.abs() + want.abs().max())).all()), (name, y0, float((got - want).abs().max()))
    # non-vacuity: the target 2^31 bytes earlier gives other last-row gradients
    y0 = LH - 4
    crop = [None if t is None else t[:, y0:y0 + 4].double().cpu().requires_grad_() for t in maps_d]
    ref = O.cook_torrance(*crop, None, view=torch.tensor(kw["view_dir"], dtype=torch.float64), light=torch.tensor(L[0]), intensity=torch.tensor(I[0]),
                          light_type="point", light_size=kw["light_size"], y_offset=y0, H_total=LH)
    ((ref - target[:, y0 - SIGNED_SHIFT:y0 + 4 - SIGNED_SHIFT].double().cpu()) ** 2).sum().div(n).backward()
    want = host[0][:, y0:y0 + 4].double()
    _distinct(want.numpy(), crop[0].grad.numpy(), float((2e-5 * (want.abs() + want.abs().max())).max()), "limit mse step")


def test_scalar_bases_at_their_limit_repeat_inner():
    """tile(2) of 16376 x 16384 fp32 maps: the 32752 x 32768 image through the repeat-inner walk (forward) and the folded backward, whose
    32-bit lane offsets into the result / upstream reach 2^31 bytes in the first repeat and whose uniform repeat offsets go past 2^32 bytes.
    Forward and map-sized gradients bit-equal to scalar_base = 0; first and last rows of the image, and the first and last map rows' gradients
    (summed over their 4 repeats) against float64.  Measured peak 60 GiB."""
    from pypbr_amd import functional as F
    _need(68)
    mh, mw, tile = LH // 2, LW // 2, (2, 2)
    maps = _maps(mh, mw, 53)
    kw = _kw("point")
    plan = F.plan_cook_torrance(*maps, tile=tile, **kw)
    assert plan.kernel_name.startswith("ctr_"), plan.kernel_name
    got = plan.launch().reshape(3, LH, LW)
    del plan
    assert torch.equal(got, F.cook_torrance(*maps, tile=tile, tuning={"scalar_base": 0}, **kw).reshape(3, LH, LW))
    for y0 in _window_rows():
        ref = _parity(got[:, y0:y0 + 4], _tiled_rows(maps, y0, 4, tile), kw, y0, LH, ("limit repeat-inner", y0))
    y1 = LH - 4 - SIGNED_SHIFT
    _distinct(ref, _ref64(_tiled_rows(maps, y1, 4, tile), kw, y1, LH), TOL, "limit repeat-inner")
    del got
    gout = torch.rand(3, LH, LW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(54)).sub_(0.4)
    leaves = [t.clone().requires_grad_() for t in maps]

    def grads(tuning):
        for t in leaves:
            t.grad = None
        out = F.cook_torrance(*leaves, tile=tile, tuning=tuning, **kw)
        out.backward(gout.reshape(out.shape))
        del out
        return [t.grad for t in leaves]
    host = [g.cpu() for g in grads(None)]
    for name, g, h in zip(("albedo", "normal", "roughness", "metallic"), grads({"scalar_base": 0}), host):
        _equal_to_host(g, h, name)
    # map rows [r0, r0 + 4): image rows r and r + mh, each over both horizontal repeats; the first and the last 4 rows
    for r0 in (0, mh - 4):
        want, mag = _fold_window_ref(maps, gout, r0, kw, LH)
        for name, h, w, m in zip(("albedo", "normal", "roughness", "metallic"), host, want, mag):
            got_w = h[:, r0:r0 + 4].double()
            assert bool(((got_w - w).abs() <= _fold_bound(m, 4)).all()), (name, r0, float((got_w - w).abs().max()))
    # non-vacuity: the upstream 2^31 bytes (16384 image rows) before each repeat's rows gives the last map rows other gradients
    wrong, _ = _fold_window_ref(maps, gout, mh - 4, kw, LH, up_shift=SIGNED_SHIFT)
    _distinct(want[0].numpy(), wrong[0].numpy(), float(_fold_bound(mag[0], 4).max()), "limit repeat-inner backward")


def _fold_bound(mag, n_rep):
    """A folded texel gradient: each of its n_rep repeats within the per-pixel criterion 2e-5 (1 + |g_k|), plus fp32 rounding of the
    n_rep-term sum, n_rep * 2^-24 * sum |g_k|."""
    return 2e-5 * (n_rep + mag) + n_rep * 2.0 ** -24 * mag


def _fold_window_ref(maps, gout, r0, kw, H_total, up_shift=0):
    """float64 autograd for map rows [r0, r0 + 4) of tile(2, 2) maps [C, mh, mw]: image rows r0 + ry * mh (ry = 0, 1), both horizontal repeats,
    against the upstream rows `up_shift` earlier (cyclically); returns the folded gradients and the sums of their repeats' magnitudes."""
    mh, mw = maps[0].shape[-2:]
    crop = _tiled_rows(maps, r0, 4, (1, 2))
    want, mag = [0.0] * len(crop), [0.0] * len(crop)
    L, I = _lights(kw)
    for y0 in (r0, r0 + mh):
        rep = [t.double().requires_grad_() for t in crop]
        ref = O.cook_torrance(*rep, None, view=torch.tensor(kw["view_dir"], dtype=torch.float64), light=torch.tensor(L[0]), intensity=torch.tensor(I[0]),
                              light_type=kw["light_type"], light_size=kw["light_size"], y_offset=y0, H_total=H_total)
        yu = (y0 - up_shift) % H_total
        (ref * gout[:, yu:yu + 4].double().cpu()).sum().backward()
        for i, t in enumerate(rep):
            gk = t.grad.reshape(t.shape[0], 4, 2, mw)
            want[i] = want[i] + gk.sum(2)
            mag[i] = mag[i] + gk.abs().sum(2)
    return want, mag


# ---------------------------------------------------------------- (e) past 2^31 elements: batched launches and the map ops
def test_batch_past_2_to_31_elements_backward_fp16():
    """Backward of 12 x 8192^2 fp16 maps (the forward test's shape in test_gpu_full_shapes.py): material 11's planes start 2.2e9 elements into
    their tensors, its upstream gradient 2.2e9 floats in.  Per-lane 64-bit addresses (a batch: no scalar bases).  The first and the last
    material's first / last rows against float64 autograd; the last material's gradient differs from the one material 0 would get."""
    from pypbr_amd import functional as F
    _need(48)
    B, H, W = 12, 8192, 8192
    maps = [t.requires_grad_() for t in _maps(H, W, 61, torch.float16, B=B)]
    assert maps[0][B - 1].storage_offset() > 2 ** 31
    kw = _kw("point")
    gout = torch.rand(B, 3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(62)).sub_(0.4)
    out = F.cook_torrance(*maps, **kw)
    out.backward(gout)
    del out
    L, I = _lights(kw)

    def ref_window(b, y0, upstream):
        crop = [t[b, :, y0:y0 + 4].detach().double().cpu().requires_grad_() for t in maps]
        ref = O.cook_torrance(*crop, None, view=torch.tensor(kw["view_dir"], dtype=torch.float64), light=torch.tensor(L[0]), intensity=torch.tensor(I[0]),
                              light_type="point", light_size=kw["light_size"], y_offset=y0, H_total=H)
        (ref * upstream.double().cpu()).sum().backward()
        return [t.grad for t in crop]
    for b, y0 in ((0, 0), (B - 1, 0), (B - 1, H - 4)):
        want = ref_window(b, y0, gout[b, :, y0:y0 + 4])
        for name, t, w in zip(("albedo", "normal", "roughness", "metallic"), maps, want):
            got = t.grad[b, :, y0:y0 + 4].double().cpu()
            assert bool(((got - w).abs() <= 1e-3 * (1e-3 + w.abs()) + 2e-5 * (1 + w.abs())).all()), (name, b, y0, float((got - w).abs().max()))
    wrong = ref_window(B - 1, H - 4, gout[0, :, H - 4:])            # the upstream of material 0: where a wrapped material offset would read
    _distinct(want[0].numpy(), wrong[0].numpy(), float((1e-3 * (1e-3 + want[0].abs()) + 2e-5 * (1 + want[0].abs())).max()), "batch backward")


def test_batch_past_2_to_31_elements_mse_step():
    """The rendering-loss step over 12 x 8192^2 fp32 maps without a normal map: the last material's target starts 2.2e9 floats in.  Loss within
    1e-5 (relative) of the float64 mean over the library's own forward result; the last material's last rows' gradients against float64."""
    from pypbr_amd import functional as F
    _need(50)
    B, H, W = 12, 8192, 8192
    maps = [None if t is None else t.requires_grad_() for t in _maps(H, W, 71, B=B, normal=False)]
    kw = _kw("point")
    target = torch.rand(B, 3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(72))
    assert target[B - 1].storage_offset() > 2 ** 31
    loss = F.rendering_loss_mse(*maps, target=target, **kw)
    loss.backward()
    maps_d = [None if t is None else t.detach() for t in maps]
    n = target.numel()
    with torch.no_grad():
        loss64 = 0.0
        for b in range(B):
            out = F.cook_torrance(*[None if t is None else t[b] for t in maps_d], **kw)
            loss64 += float(((out.double() - target[b].double()) ** 2).sum())
        loss64 /= n
    assert abs(float(loss.detach()) - loss64) <= 1e-5 * loss64, (float(loss.detach()), loss64)
    L, I = _lights(kw)

    def ref_window(b, y0, tgt):
        crop = [None if t is None else t[b, :, y0:y0 + 4].double().cpu().requires_grad_() for t in maps_d]
        ref = O.cook_torrance(*crop, None, view=torch.tensor(kw["view_dir"], dtype=torch.float64), light=torch.tensor(L[0]), intensity=torch.tensor(I[0]),
                              light_type="point", light_size=kw["light_size"], y_offset=y0, H_total=H)
        ((ref - tgt.double().cpu()) ** 2).sum().div(n).backward()
        return [None if t is None else t.grad for t in crop]
    for b, y0 in ((0, 0), (B - 1, H - 4)):
        want = ref_window(b, y0, target[b, :, y0:y0 + 4])
        for name, t, w in zip(("albedo", "normal", "roughness", "metallic"), maps, want):
            if t is None:
                continue
            got = t.grad[b, :, y0:y0 + 4].double().cpu()
            assert bool(((got - w).abs() <= 2e-5 * (w.abs() + w.abs().max())).all()), (name, b, y0, float((got - w).abs().max()))
    wrong = ref_window(B - 1, H - 4, target[0, :, H - 4:])
    _distinct(want[0].numpy(), wrong[0].numpy(), float((2e-5 * (want[0].abs() + want[0].abs().max())).max()), "batch mse step")


def test_map_ops_past_2_to_31_elements():
    """The element-wise map ops on one [3, 32768, 32768] tensor (3.2e9 elements, the last plane from 2.1e9 on): sRGB <-> linear, decode_normal,
    metallic -> diffuse / specular and blend_maps, fp32.  The last elements and the first against the float64 C oracle (blend_maps: the formula
    in float64).  A plane holds exactly 2^30 elements, so a 32-bit byte offset that wrapped would reach the same window of the plane before:
each plane's far window must differ from that one."""
    from pypbr_amd import functional as F
    from pypbr_amd.blending import blend_maps
    _need(60)
    S = 32768
    g = torch.Generator(device="cuda").manual_seed(81)
    x = torch.rand(3, S, S, device="cuda", generator=g)
    assert x.numel() > 2 ** 31

    def windows(t):                                                   # first row's first 4096 columns, last row's last 4096 columns
        return t[..., 0, :4096].double().cpu().numpy(), t[..., -1, -4096:].double().cpu().numpy()

    def check(got, want_fn, src, tol, what):
        for gw, sw in zip(windows(got), windows(src)):
            assert np.abs(gw - want_fn(sw)).max() <= tol, what
        far = windows(got)[1]
        _distinct(far[1:], far[:-1], tol, what)
    check(F.srgb_to_linear(x), lambda s: C.srgb_to_linear(s[:, None], np.float64)[:, 0], x, 2e-6, "srgb_to_linear")
    check(F.linear_to_srgb(x), lambda s: C.linear_to_srgb(s[:, None], np.float64)[:, 0], x, 2e-6, "linear_to_srgb")
    n = F.decode_normal(x)
    for gw, sw in zip(windows(n), windows(x)):
        assert np.abs(gw - C.decode_normal(sw[:, None], np.float64)[:, 0]).max() <= 2e-6, "decode_normal"
    _distinct(windows(n)[1][1:], windows(n)[1][:-1], 2e-6, "decode_normal")
    del n
    m = x[:1].clone()
    d, s = F.metallic_to_diffuse_specular(x, m)
    for gd, gs, sa, sm in zip(windows(d), windows(s), windows(x), windows(m)):
        wd, ws = C.metallic_to_specular(sa[:, None], sm[:, None], np.float64)
        assert np.abs(gd - wd[:, 0]).max() <= 2e-6 and np.abs(gs - ws[:, 0]).max() <= 2e-6, "metallic_to_diffuse_specular"
    _distinct(windows(d)[1][1:], windows(d)[1][:-1], 2e-6, "metallic_to_diffuse_specular")
    del d, s
    y = torch.rand(3, S, S, device="cuda", generator=g)
    b = blend_maps(x, y, m)
    for gw, xa, ya, ma in zip(windows(b), windows(x), windows(y), windows(m)):
        assert np.abs(gw - (ma * xa + (1 - ma) * ya)).max() <= 2e-6, "blend_maps"
    _distinct(windows(b)[1][1:], windows(b)[1][:-1], 2e-6, "blend_maps")


# ---------------------------------------------------------------- (e) resize: every form pbr_resize_form selects, the last plane past 2^31
RP, RS = 130, 4096                  # 130 planes of 4096^2: plane 129 starts at 2.16e9 elements; 2^30 elements (2^32 bytes) before it is plane 65


def _interp64(plane, size, gout=None, antialias=True, dtype=torch.float64):
    """F.interpolate (bilinear, align_corners=False) of one [H, W] plane in `dtype` on the host; with `gout`, also the gradient w.r.t. the plane."""
    x = plane.to(dtype).cpu()[None, None].requires_grad_(gout is not None)
    y = torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=antialias)
    if gout is None:
        return y[0, 0].detach(), None
    (y * gout.to(dtype).cpu()[None, None]).sum().backward()
    return y[0, 0].detach().double(), x.grad[0, 0].double()


@pytest.mark.parametrize("size,form", [((4100, 4100), "TWO_TAP"), ((2048, 2048), "BAND_WALK"), ((400, 400), "ROW_WALK"),
                                       ((700, 700), "STRIP"), ((100, 100), "TWO_PASS")])
def test_resize_past_2_to_31_elements(size, form):
    """MaterialBase.resize of 130 planes of 4096^2, forward and backward, in each form pbr_resize_form names for the shape (the row walk is the
    streamed form, resize_stream.hpp); antialiased down-scales, a plain bilinear up-scale.  Planes 0 and 129 against float64 F.interpolate and
    its autograd -- the up-scale against ATen's fp32 F.interpolate instead: 4096 -> 4100 puts its source coordinates at x * (4096 / 4100) with
    the scale rounded to fp32 (ATen's arithmetic, kept by the kernel), up to 2e-4 from the float64 evaluation -- under the criteria of test_gpu_map_op_gradients.py (1e-5; 2e-5 (1 + |g|)); plane 129's result and input gradient differ from
    plane 65's, where an offset wrapped at 2^32 bytes would land.  Measured peak 41 GiB (the up-scale)."""
    from pypbr_amd import _native as N, functional as F
    _need(46)
    g = torch.Generator(device="cuda").manual_seed(90 + size[0])
    x = torch.rand(RP, RS, RS, device="cuda", generator=g).requires_grad_()
    aa = form != "TWO_TAP"
    out = F.resize(x, size, antialias=aa)
    assert out.shape == (RP,) + size
    assert N.lib().pbr_resize_form(x.data_ptr(), out.data_ptr(), RP, RS, RS, size[0], size[1], int(aa), x.data_ptr()) == getattr(N, "RESIZE_" + form)
    gout = torch.rand(out.shape, device="cuda", generator=g).sub_(0.4)
    out.backward(gout)
    gin = x.grad
    refs = {}
    for p in (0, RP - 1, RP - 1 - 64):
        refs[p] = _interp64(x[p].detach(), size, gout[p], aa, torch.float64 if aa else torch.float32)
    for p in (0, RP - 1):
        y64, g64 = refs[p]
        assert float((out[p].detach().double().cpu() - y64).abs().max()) <= 1e-5, (form, p)
        gtol = 2e-5 * (1 + g64.abs())
        assert bool(((gin[p].double().cpu() - g64).abs() <= gtol).all()), (form, p, float((gin[p].double().cpu() - g64).abs().max()))
    far, wrapped = refs[RP - 1], refs[RP - 1 - 64]
    _distinct(far[0].numpy(), wrapped[0].numpy(), 1e-5, ("resize", form))
    _distinct(far[1].numpy(), wrapped[1].numpy(), float((2e-5 * (1 + far[1].abs())).max()), ("resize backward", form))


# ---------------------------------------------------------------- (e) the image unpack
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("decode", [False, True], ids=["plain", "normal"])
def test_unpack_image_past_2_to_31_elements(bits, decode):
    """MaterialBase._to_tensor (and the fused normal decode) of a 32768^2 RGB image with 8- and 16-bit samples: the float32 (3, H, W) result holds
    3.2e9 elements, plane 2 from 2^31 on, and a plane is exactly 2^30 elements (2^32 bytes).  The first and the far windows: plain samples equal
    the host formula float32(v) / float32(2^bits - 1) exactly (IEEE division, as the kernel); decoded normals within 2e-6 of the float64 oracle.
    Each plane's far window differs from the plane before's (where a wrapped offset would land)."""
    from pypbr_amd import functional as F
    _need(24)
    S, Cn = 32768, 3
    g = torch.Generator(device="cuda").manual_seed(100 + bits)
    if bits == 8:
        samples = torch.randint(0, 256, (S, S, Cn), device="cuda", generator=g, dtype=torch.uint8)
    else:
        samples = torch.randint(-32768, 32768, (S, S, Cn), device="cuda", generator=g, dtype=torch.int16)   # read as unsigned 16-bit samples
    out = torch.empty(3, S, S, device="cuda")
    F.unpack_image(samples, bits, (1, S * Cn, Cn), (Cn, S, S), out, decode_normal=decode)
    div = np.float32(2 ** bits - 1)

    def host(win):                     # (n, C) samples -> (C, n) float32
        v = win.cpu().numpy()
        v = v.view(np.uint16) if bits == 16 else v
        return (v.astype(np.float32) / div).T
    wins = [(0, slice(0, 4096)), (S - 1, slice(S - 4096, S))]
    for y, xs in wins:
        got = out[:, y, xs].cpu().numpy()
        want = host(samples[y, xs])
        if decode:
            ref = C.decode_normal(want.astype(np.float64)[:, None, :], np.float64)[:, 0]
            assert np.abs(got - ref).max() <= 2e-6, (bits, y)
        else:
            assert np.array_equal(got, want), (bits, y)
    far = out[:, S - 1, S - 4096:].cpu().numpy()
    _distinct(far[1:], far[:-1], 2e-6, ("unpack", bits, decode))


# ---------------------------------------------------------------- (e) fold_gradient
def test_fold_gradient_past_2_to_31_elements():
    """pbr_fold_gradient_typed (the sum over the repeats of tile(2)) of a [1, 3, 32768, 32768] fp32 gradient, 3.2e9 elements, each channel plane
    exactly 2^30 elements.  Channel 0's first rows and channel 2's last rows against the float64 sum (bound: 4 * 2^-24 * sum |terms|); each far
    window differs from the one a wrap of 2^32 bytes would read (the channel before)."""
    from pypbr_amd import _native as N, functional as F
    _need(20)
    h = w = 16384
    src = torch.rand(1, 3, 2 * h, 2 * w, device="cuda", generator=torch.Generator(device="cuda").manual_seed(111)).sub_(0.5)
    dst = torch.empty(1, 3, h, w, device="cuda")
    with torch.cuda.device(src.device):
        N.check(N.lib().pbr_fold_gradient_typed(src.data_ptr(), dst.data_ptr(), 1, 3, h, w, 2, 2, 0, N.F32, F._stream_ptr(src.device)))

    def ref(c, r0):
        terms = [src[0, c, ty * h + r0:ty * h + r0 + 4, tx * w:(tx + 1) * w].double().cpu() for ty in (0, 1) for tx in (0, 1)]
        return sum(terms), sum(t.abs() for t in terms)
    for c, r0 in ((0, 0), (2, h - 4)):
        want, mag = ref(c, r0)
        assert bool(((dst[0, c, r0:r0 + 4].double().cpu() - want).abs() <= 4 * 2.0 ** -24 * mag).all()), (c, r0)
    far, _ = ref(2, h - 4)
    _distinct(far.numpy(), ref(1, h - 4)[0].numpy(), float(4 * 2.0 ** -24 * 4), "fold_gradient")


# ---------------------------------------------------------------- (e) a batch of tiled materials: forward and folded backward
def test_batch_of_tiled_materials_past_2_to_31_elements():
    """tile(2) of 4 materials of 8192^2 fp32 maps: a [4, 3, 16384, 16384] result whose last material starts 2.4e9 elements in.  The repeat-inner
    walk over a batch addresses per lane; scalar_base = 2 (scalar bases wherever the launch allows them, its planes are < 2^30) is the second
    form: result and folded gradients bit-equal to it.  Material 0's first rows and material 3's last rows against float64 (forward: the parity
    criterion; gradients: 4 repeats, _fold_bound); material 3's far windows differ from material 0's.  Peak about 40 GiB."""
    from pypbr_amd import functional as F
    _need(48)
    B, mh, mw, tile = 4, 8192, 8192, (2, 2)
    H, W = 2 * mh, 2 * mw
    maps = _maps(mh, mw, 121, B=B)
    kw = _kw("point")
    got = F.cook_torrance(*maps, tile=tile, **kw)
    assert got.shape == (B, 3, H, W) and got[B - 1].storage_offset() > 2 ** 31
    assert torch.equal(got, F.cook_torrance(*maps, tile=tile, tuning={"scalar_base": 2}, **kw))
    refs = {}
    for b, y0 in ((0, 0), (B - 1, H - 4), (0, H - 4)):
        mb = [t[b] for t in maps]
        if b == B - 1 or y0 == 0:
            refs[b, y0] = _parity(got[b, :, y0:y0 + 4], _tiled_rows(mb, y0, 4, tile), kw, y0, H, ("batch tiled", b, y0))
        else:
            refs[b, y0] = _ref64(_tiled_rows(mb, y0, 4, tile), kw, y0, H)
    _distinct(refs[B - 1, H - 4], refs[0, H - 4], TOL, "batch tiled forward")
    del got
    gout = torch.rand(B, 3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(122)).sub_(0.4)
    for t in maps:
        t.requires_grad_()

    def grads(tuning):
        for t in maps:
            t.grad = None
        out = F.cook_torrance(*maps, tile=tile, tuning=tuning, **kw)
        out.backward(gout)
        del out
        return [t.grad for t in maps]
    host = [g.cpu() for g in grads(None)]
    for name, g, h in zip(("albedo", "normal", "roughness", "metallic"), grads({"scalar_base": 2}), host):
        _equal_to_host(g, h, name)
    md = [t.detach() for t in maps]
    for b, r0 in ((0, 0), (B - 1, mh - 4)):
        want, mag = _fold_window_ref([t[b] for t in md], gout[b], r0, kw, H)
        for name, h, w_, m in zip(("albedo", "normal", "roughness", "metallic"), host, want, mag):
            got_w = h[b, :, r0:r0 + 4].double()
            assert bool(((got_w - w_).abs() <= _fold_bound(m, 4)).all()), (name, b, r0, float((got_w - w_).abs().max()))
    wrong, _ = _fold_window_ref([t[B - 1] for t in md], gout[0], mh - 4, kw, H)      # material 0's upstream
    _distinct(want[0].numpy(), wrong[0].numpy(), float(_fold_bound(mag[0], 4).max()), "batch tiled backward")


# ---------------------------------------------------------------- (e) the untiled fused blend, forward
def test_fused_blend_past_2_to_31_elements():
    """cook_torrance(blend=...) over 12 x 8192^2 fp32 materials (untiled, one pass: blend + evaluate): material 11's albedo, normal and result
    start 2.2e9 elements in.  The whole result bit-equal to scalar_base = 2 (scalar bases for the batch; its planes are < 2^30), compared through a
    host copy; material 0's first rows and material 11's last rows within 1e-5 of float64 blend + BRDF; material 11's far window differs from
    material 0's.  Peak about 60 GiB.  The blend's backward at this shape would need about 100 GiB (both materials' and the mask's gradients
    beside the maps) and is not run here."""
    from pypbr_amd import functional as F
    _need(66)
    B, H, W = 12, 8192, 8192
    m1, m2 = _maps(H, W, 131, B=B), _maps(H, W, 132, B=B)
    mask = torch.rand(B, 1, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(133))
    assert m1[0][B - 1].storage_offset() > 2 ** 31
    kw = _kw("point")
    second = (m2[0], m2[1], m2[2], m2[3], None, mask)
    got = F.cook_torrance(*m1, blend=second, **kw)
    assert got.shape == (B, 3, H, W) and got[B - 1].storage_offset() > 2 ** 31
    win = {}
    for b, y0 in ((0, 0), (B - 1, H - 4), (0, H - 4)):
        win[b, y0] = got[b, :, y0:y0 + 4].double().cpu().numpy()
    host = got.cpu()
    del got
    _equal_to_host(F.cook_torrance(*m1, blend=second, tuning={"scalar_base": 2}, **kw), host, "fused blend")
    del host
    refs = {}
    for b, y0 in ((0, 0), (B - 1, H - 4), (0, H - 4)):
        refs[b, y0] = _blend_ref64([t[b] for t in m1], [t[b] for t in m2], mask[b], y0, 4, (1, 1), kw)
    for key in ((0, 0), (B - 1, H - 4)):
        assert np.abs(win[key] - refs[key]).max() <= TOL, key
    _distinct(refs[B - 1, H - 4], refs[0, H - 4], TOL, "fused blend")
