"""Addressing and table limits that launch nothing (no GPU): the functions of the library that only DECIDE -- pbr_smoothness_check,
pbr_smoothness_workspace_bytes, pbr_adam_check, and the Python-side validators -- at their documented boundaries and one step inside them, and the
photometric-stereo populations of tests/test_gpu_addressing_limits_capture_fit.py under the light counts no other test runs.

The decisions: a height or a width of 2^30 is taken, 2^30 + 1 refused; H W = 2^40 is taken, more refused; a launch of 2^31 - 2^15
workgroups is taken (and its workspace is four bytes for each), one of 2^31 refused; every negative stride is refused; and the interval
test of adam.hip and smoothness.hip sees planes whose distance is a stride past 2^32 bytes where they are: a written plane at
base + stride overlaps what lies THERE, and does not overlap what lies at base + (stride mod 2^32 bytes), where 32-bit arithmetic
would put it.  The pointers are never dereferenced: the functions called here cannot launch.

Photometric populations (tools/photometric_cases.py with n_lights = 3, 4, 16; float64 oracle at the defaults), 24 x 36 | 24 x 35.
tests/test_photometric_host.py's rule: at most 3 of 864 pixels without a margin of 1e-4; the band of the GPU test is the smallest of
2e-6, 1e-5, 1e-4 that covers 4 x the float32 oracle's own error on the banded pixels:
  L   set        valid / invalid           margin < 1e-4   float32 oracle      band
  3   gentle     799 / 65 | 778 / 62       0 | 1           6.3e-7 | 5.2e-7     1e-5 | 1e-5
  3   shadowed   368 / 496 | 356 / 484     2 | 0           4.2e-7 | 4.5e-7     2e-6 | 2e-6
  4   gentle     860 / 4 | 836 / 4         0 | 0           4.2e-7 | 4.2e-7     2e-6 | 2e-6
  4   shadowed   647 / 217 | 631 / 209     1 | 1           1.8e-6 | 1.6e-6     1e-5 | 1e-5
  16  gentle     864 / 0 | 840 / 0         1 | 1           5.5e-7 | 5.5e-7     1e-5 | 1e-5
  16  shadowed   864 / 0 | 840 / 0         3 | 1           8.6e-7 | 8.0e-7     1e-5 | 1e-5
(three lights leave no shot to spare: a pixel that loses one to the shadow mask has no solution.)  The shadowed set of L = 8 under
iterations = 1 ... 4: the same rule, recorded in ITERATIONS below (K = 1: 3.5e-7 | 3.6e-7 -> 2e-6; K = 2: 6.6e-7 | 5.9e-7 -> 1e-5; K = 3, 4: 1.3e-6 | 2.1e-6
-> 1e-5)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import photometric_cases as C  # noqa: E402
import photometric_oracle as O  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402
from test_photometric_host import band_for, float32_error  # noqa: E402

TWO32 = 1 << 32


def _lib():
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libpbr_hip.so is not built")
    return N.lib()


# ---------------------------------------------------------------- smoothness: pbr_smoothness_check / pbr_smoothness_workspace_bytes
def smooth(param=0x10000000, grad=None, weights=None, pbs=0, pps=None, gbs=0, gps=None, wbs=0, dtype=None, batch=1, channels=1, height=8, width=8,
           kind=N.SMOOTH_L2, wrap=0):
    plane = height * width
    return N.SmoothTensor(param, grad, weights, pbs, plane if pps is None else pps, gbs, plane if gps is None else gps, wbs, 1.0, 1e-3,
                          N.F32 if dtype is None else dtype, batch, channels, height, width, kind, wrap)


def smooth_check(*entries):
    table = (N.SmoothTensor * len(entries))(*entries)
    lib = _lib()
    return lib.pbr_smoothness_check(table, len(entries)), lib.pbr_smoothness_workspace_bytes(table, len(entries))


def test_smoothness_extents_at_2_to_30_and_the_pixel_count_at_2_to_40():
    for kw in (dict(height=1 << 30, width=1), dict(height=1, width=1 << 30), dict(height=1 << 20, width=1 << 20), dict(height=1 << 30, width=1 << 10)):
        rc, nbytes = smooth_check(smooth(**kw))
        assert rc == N.OK and nbytes > 0 and nbytes % 4 == 0, kw
    for kw in (dict(height=(1 << 30) + 1, width=1), dict(height=1, width=(1 << 30) + 1), dict(height=1 << 20, width=(1 << 20) + 1),
               dict(height=(1 << 20) + 1, width=1 << 20), dict(height=1 << 30, width=(1 << 10) + 1), dict(height=0), dict(width=0), dict(height=-1)):
        assert smooth_check(smooth(**kw)) == (N.ERR_SHAPE, 0), kw


def test_smoothness_workgroups_at_2_to_31():
    """One strip group per row band (a width of 4 x 63 x 4 pixels on the quad path), 2^15 bands of 32 rows, 2^16 images: 2^31 workgroups."""
    width, height = 4 * 63 * (N.SMOOTH_BLOCK // 64), N.SMOOTH_BAND_ROWS << 15
    inside = smooth(height=height, width=width, batch=(1 << 16) - 1)
    assert smooth_check(inside) == (N.OK, 4 * ((1 << 31) - (1 << 15)))
    assert smooth_check(smooth(height=height, width=width, batch=1 << 16)) == (N.ERR_SHAPE, 0)
    # the sum over the entries of a table counts, not each entry
    half = smooth(height=height, width=width, batch=1 << 15)
    assert smooth_check(half, smooth(param=0x20000000, height=height, width=width, batch=(1 << 15) - 1)) == (N.OK, 4 * ((1 << 31) - (1 << 15)))
    assert smooth_check(half, smooth(param=0x20000000, height=height, width=width, batch=1 << 15)) == (N.ERR_SHAPE, 0)
    # one column more is a second strip group: twice the workgroups
    assert smooth_check(smooth(height=height, width=width + 4, batch=1 << 15)) == (N.ERR_SHAPE, 0)
    assert smooth_check(smooth(height=height, width=width + 4, batch=(1 << 15) - 1))[0] == N.OK


def test_smoothness_negative_strides():
    for name in ("pbs", "pps", "gbs", "gps", "wbs"):
        kw = dict(grad=0x20000000, weights=0x30000000, batch=2, channels=2, pbs=256, gbs=256)
        assert smooth_check(smooth(**dict(kw, **{name: -64})))[0] == N.ERR_SHAPE, name
        assert smooth_check(smooth(**dict(kw, **{name: 1024})))[0] == N.OK, name


@pytest.mark.parametrize("dtype,esz", [(N.F32, 4), (N.F16, 2)], ids=["fp32", "fp16"])
def test_smoothness_intervals_past_2_to_32_bytes(dtype, esz):
    """A gradient of two images whose batch stride is 2^32 bytes + 4096: image 1 lies at base + 2^32 + 4096, not at base + 4096."""
    base, plane = 0x7f0000000000, 64 * esz
    stride = (TWO32 + 4096) // esz
    far, wrapped = base + TWO32 + 4096, base + 4096
    kw = dict(grad=base, gbs=stride, batch=2, dtype=dtype)
    # the parameter (only read, but the gradient is written) placed on the gradient's second image, and just beside it
    for param, want in ((far, N.ERR_SHAPE), (far + plane - esz, N.ERR_SHAPE), (far - plane + esz, N.ERR_SHAPE), (far + plane, N.OK), (far - 2 * plane, N.OK),
                        (wrapped, N.OK), (base + plane, N.OK), (base, N.ERR_SHAPE)):
        assert smooth_check(smooth(param=param, pbs=0, **kw))[0] == want, hex(param - base)
    # the same for a plane stride, and for weights per image
    kw = dict(grad=base, gps=stride, channels=2, dtype=dtype, param=base + 3 * TWO32)
    for weights, want in ((far, N.ERR_SHAPE), (wrapped, N.OK), (far + plane, N.OK)):
        assert smooth_check(smooth(weights=weights, **kw))[0] == want, hex(weights - base)
    # a second entry's gradient on the first one's far image
    first = smooth(param=base + 3 * TWO32, grad=base, gbs=stride, batch=2, dtype=dtype)
    for grad, want in ((far, N.ERR_SHAPE), (wrapped, N.OK)):
        assert smooth_check(first, smooth(param=base + 4 * TWO32, grad=grad, dtype=dtype))[0] == want, hex(grad - base)
    # a parameter whose own stride passes 2^32 bytes reaches the gradient only where it really lies
    for grad, want in ((far, N.ERR_SHAPE), (wrapped, N.OK)):
        assert smooth_check(smooth(param=base, pbs=stride, batch=2, grad=grad, gbs=2 * TWO32 // esz, dtype=dtype))[0] == want, hex(grad - base)


# ---------------------------------------------------------------- adam: pbr_adam_check
def adam(param=0x7f0000000000, grad=0x7e0000000000, m=0x7d0000000000, v=0x7c0000000000, master=None, pixels=64, pbs=0, pps=None, gbs=0, gps=None, batch=1,
         channels=1, dtype=N.F32, project=N.ADAM_NONE):
    return N.AdamTensor(param, grad, m, v, master, pixels, pbs, pixels if pps is None else pps, gbs, pixels if gps is None else gps, batch, channels, dtype,
                        project, 0.0, 1.0, 0.0, 0)


def adam_check(*entries):
    return _lib().pbr_adam_check((N.AdamTensor * len(entries))(*entries), len(entries), 1)


def test_adam_negative_strides_and_planes_on_top_of_each_other():
    assert adam_check(adam(batch=2, channels=2, pbs=256, gbs=256)) == N.OK
    for name in ("pbs", "pps", "gbs", "gps"):
        assert adam_check(adam(batch=2, channels=2, **dict(dict(pbs=256, gbs=256), **{name: -256}))) == N.ERR_SHAPE, name
    assert adam_check(adam(channels=2, pps=63)) == N.ERR_SHAPE and adam_check(adam(batch=2, channels=2, pbs=127)) == N.ERR_SHAPE
    assert adam_check(adam(batch=2, channels=2, pbs=128, gbs=0, gps=0)) == N.OK          # the gradient is only read: an expanded one
    assert adam_check(adam(pixels=0)) == N.ERR_SHAPE


@pytest.mark.parametrize("dtype,esz", [(N.F32, 4), (N.F16, 2)], ids=["fp32", "fp16"])
def test_adam_intervals_past_2_to_32_bytes(dtype, esz):
    """A parameter of two images whose batch stride is 2^32 bytes + 4096: the state, a second parameter and the gradient collide with
    image 1 at base + 2^32 + 4096 and nowhere else."""
    base, plane = 0x7f0000000000, 64 * esz
    stride = (TWO32 + 4096) // esz
    far, wrapped = base + TWO32 + 4096, base + 4096
    master = 0x7b0000000000 if dtype == N.F16 else None
    kw = dict(param=base, pbs=stride, batch=2, dtype=dtype, master=master)
    for name in ("grad", "m", "v") + (("master",) if master else ()):
        for at, want in ((far, N.ERR_SHAPE), (far + plane - 4, N.ERR_SHAPE), (far + plane, N.OK), (wrapped, N.OK), (base + plane, N.OK), (base, N.ERR_SHAPE)):
            assert adam_check(adam(**dict(kw, **{name: at}))) == want, (name, hex(at - base))
    # the dense state of 2 x 64 floats ends 512 bytes behind its start: one byte inside that and outside it
    for at, want in ((far - 512, N.OK), (far - 508, N.ERR_SHAPE)):
        assert adam_check(adam(**dict(kw, m=at))) == want
    # plane strides, and a second entry
    kw = dict(param=base, pps=stride, channels=2, dtype=dtype, master=master)
    for at, want in ((far, N.ERR_SHAPE), (wrapped, N.OK)):
        assert adam_check(adam(**dict(kw, v=at))) == want
        assert adam_check(adam(**kw), adam(param=at, grad=0x7a0000000000, m=0x790000000000, v=0x780000000000, dtype=dtype,
                                           master=0x770000000000 if master else None)) == want
    # a gradient whose stride passes 2^32 bytes may lie on itself, never on what is written
    for at, want in ((far, N.ERR_SHAPE), (wrapped, N.OK)):
        assert adam_check(adam(grad=base, gbs=stride, batch=2, pbs=64, param=at, dtype=dtype, master=master)) == want
    # dense state past 2^31 elements: 2^20 planes of 2^12 pixels; the second state array may begin where the first ends
    big = dict(param=base, pixels=1 << 12, batch=1 << 10, channels=1 << 10, pbs=1 << 22, dtype=dtype, master=master, grad=0x7e0000000000, gbs=0, gps=0)
    state_bytes = 4 << 32
    assert adam_check(adam(m=0x700000000000, v=0x700000000000 + state_bytes, **big)) == N.OK
    assert adam_check(adam(m=0x700000000000, v=0x700000000000 + state_bytes - 4, **big)) == N.ERR_SHAPE
    assert adam_check(adam(m=0x700000000000, v=0x700000000000 + (state_bytes - 4) % TWO32 + TWO32, **big)) == N.ERR_SHAPE


# ---------------------------------------------------------------- the Python-side validators
def test_python_validators_at_their_boundaries():
    """What the wrappers decide before any device work: 16 shots pass photometric_stereo's count check (and reach the device check), 17 do
    not; optim._planes and _dispatch.rows_are_dense hand on strides past 2^32 bytes as they are and refuse rows that are not dense (torch has no negative strides to hand on); _rows_dense
    keeps a view with such strides and copies one without dense rows."""
    import torch
    from pypbr_amd import capture, priors
    from pypbr_amd._dispatch import _rows_dense, rows_are_dense
    from pypbr_amd.optim import _planes
    kw = dict(light_intensity=[1.0, 1.0, 1.0])
    assert N.MAX_PHOTOMETRIC_SHOTS == 16
    with pytest.raises(ValueError, match="ROCm"):
        capture.photometric_stereo(torch.zeros(16, 3, 8, 8), light=torch.tensor([[0.1, 0.2, 0.9]] * 16), **kw)
    with pytest.raises(ValueError, match="at most 16"):
        capture.photometric_stereo(torch.zeros(17, 3, 8, 8), light=torch.tensor([[0.1, 0.2, 0.9]] * 17), **kw)
    strides = ((1 << 33) + 4, (1 << 31) + 4, 36, 1)
    far = torch.empty_strided((2, 3, 24, 36), strides, device="meta")                      # (no storage: only the geometry is read)
    assert _planes(far) == (far, 2, 3, 864, strides[0], strides[1]) and rows_are_dense(far) and _rows_dense(far) is far
    three = torch.empty_strided((3, 24, 36), strides[1:], device="meta")
    assert _planes(three) == (three, 1, 3, 864, 0, strides[1])
    t = torch.zeros(2, 3, 24, 36)
    for view in (t.transpose(-1, -2), t[..., ::2], t[:, :, ::2]):                             # rows that are not dense: refused, or copied
        assert _planes(view) is None and not rows_are_dense(view) and _rows_dense(view).is_contiguous()
    assert _planes(t.expand(4, 2, 3, 24, 36)[0]) is not None and _planes(t[:, :1].expand(2, 3, 24, 36))[5] == 0      # an expanded plane: stride 0 is forwarded
    smooth_entry = priors._entry(far, far, None, 1.0, N.SMOOTH_L2, 1e-3, False)
    assert (smooth_entry.param_batch_stride, smooth_entry.param_plane_stride, smooth_entry.grad_plane_stride) == (strides[0], strides[1], strides[1])


# ---------------------------------------------------------------- the photometric populations of the new light counts
SIZES = (C.SIZE, C.SIBLING)
EXPECTED = {    # (lights, name, width) -> (valid, invalid, pixels with margin < 1e-4, the float32 oracle's error on the banded pixels)
    (3, "gentle", 36): (799, 65, 0, 6.3e-7), (3, "gentle", 35): (778, 62, 1, 5.2e-7),
    (3, "shadowed", 36): (368, 496, 2, 4.2e-7), (3, "shadowed", 35): (356, 484, 0, 4.5e-7),
    (4, "gentle", 36): (860, 4, 0, 4.2e-7), (4, "gentle", 35): (836, 4, 0, 4.2e-7),
    (4, "shadowed", 36): (647, 217, 1, 1.8e-6), (4, "shadowed", 35): (631, 209, 1, 1.6e-6),
    (16, "gentle", 36): (864, 0, 1, 5.5e-7), (16, "gentle", 35): (840, 0, 1, 5.5e-7),
    (16, "shadowed", 36): (864, 0, 3, 8.6e-7), (16, "shadowed", 35): (840, 0, 1, 8.0e-7),
}
ITERATIONS = {  # (iterations, width) of the shadowed set, L = 8 -> the float32 oracle's error on the banded pixels
    (1, 36): 3.5e-7, (1, 35): 3.6e-7, (2, 36): 6.6e-7, (2, 35): 5.9e-7, (3, 36): 1.3e-6, (3, 35): 2.1e-6, (4, 36): 1.3e-6, (4, 35): 2.1e-6,
}
MAX_WITHOUT_MARGIN = 3          # of 864 (tests/test_photometric_host.py's rule)


@functools.lru_cache(maxsize=None)
def case(name, size=C.SIZE, n_lights=C.N_LIGHTS):
    return C.lambertian(name, size, n_lights=n_lights)


@functools.lru_cache(maxsize=None)
def solved(name, size=C.SIZE, n_lights=C.N_LIGHTS, dtype=np.float64, **kw):
    c = case(name, size, n_lights)
    return O.photometric_stereo(c.targets, c.weights, c.light, c.intensity, light_size=C.LIGHT_SIZE, dtype=dtype, **kw)


def band(name, size, n_lights=C.N_LIGHTS, **kw):
    """The band of the GPU test: from the recorded float32 error, which the tests below hold within 25 % of today's."""
    recorded = EXPECTED[(n_lights, name, size[1])][3] if not kw else ITERATIONS[(kw["iterations"], size[1])]
    return band_for(recorded)


def test_the_existing_sets_are_what_they_were():
    """n_lights defaults to 8: the generator's own sets, bit for bit (tests/test_photometric_host.py pins their counts)."""
    eight = C.lights(C.SETS["gentle"][1])
    assert np.array_equal(C.lights(C.SETS["gentle"][1], 8), eight) and eight.shape == (8, 3)
    assert np.array_equal(C.partial_weights(), C.partial_weights(C.SIZE, 8))
    for name in ("gentle", "shadowed", "partial"):
        a, b = C.lambertian(name), C.lambertian(name, n_lights=8)
        assert all(x is y is None or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["gentle", "shadowed"])
@pytest.mark.parametrize("n_lights", [3, 4, 16])
def test_populations_of_the_other_light_counts(n_lights, name, size):
    c, r = case(name, size, n_lights), solved(name, size, n_lights)
    assert c.targets.shape == (n_lights, 3) + size and c.targets.dtype == np.float32 and 0 <= c.targets.min() and c.targets.max() < 1
    assert c.light.shape == (n_lights, 3) and len({tuple(row) for row in c.light.tolist()}) == n_lights
    clear, _, banded = C.classes(r)
    valid, invalid, unclear = int(r.valid.sum()), int((~r.valid).sum()), int((~clear).sum())
    r32 = solved(name, size, n_lights, np.float32)
    err = float32_error(r32, r)
    print("L=%d %s %s: valid %d invalid %d  margin < 1e-4: %d  banded %d  float32 oracle %.2e -> band %.0e"
          % (n_lights, name, size, valid, invalid, unclear, int(banded.sum()), err, band_for(err)))
    want = EXPECTED[(n_lights, name, size[1])]
    assert (valid, invalid, unclear) == want[:3]
    assert unclear <= MAX_WITHOUT_MARGIN and banded.sum() >= 300
    assert np.array_equal(r32.valid[clear], r.valid[clear])
    assert err <= 1.25 * want[3] and band_for(err) == band_for(want[3])


@pytest.mark.parametrize("size", SIZES)
def test_sixteen_lights_drop_shots_of_the_upper_half_of_the_mask(size):
    """Bits 8 ... 15 of the kernel's shadow mask: pixels whose final solution leaves out a shot with index >= 8, and pixels whose set of
    such shots changes between the second and the third pass."""
    r2, r3 = solved("shadowed", size, 16, iterations=2), solved("shadowed", size, 16)
    dropped = r3.valid[None] & ~r3.used
    moved = (r2.valid & r3.valid)[None] & (r2.used != r3.used)
    print("L=16 shadowed %s: %d pixels drop a shot >= 8, %d change one between passes 2 and 3; shot 15 dropped at %d"
          % (size, int(dropped[8:].any(axis=0).sum()), int(moved[8:].any(axis=0).sum()), int(dropped[15].sum())))
    assert dropped[8:].any(axis=0).sum() >= 100 and dropped[15].sum() >= 10 and dropped[:8].any(axis=0).sum() >= 100
    assert moved[8:].any(axis=0).sum() >= 10


@pytest.mark.parametrize("n_lights", [3, 4])
def test_the_solvable_minimum_and_one_shot_masked_by_weight(n_lights):
    c = case("gentle", C.SIZE, n_lights)
    r = solved("gentle", C.SIZE, n_lights)
    assert r.valid.mean() > 0.9 and (r.confidence[r.valid] > 0.05).all()
    weights = masked_weights(n_lights)
    m = O.photometric_stereo(c.targets, weights, c.light, c.intensity, light_size=C.LIGHT_SIZE)
    left = np.zeros(C.SIZE, bool)
    left[:, :C.SIZE[1] // 2] = True
    clear, _, banded = C.classes(m)
    if n_lights == 3:
        assert not m.valid[left].any() and (m.confidence[left] == 0).all() and (m.margin[left] >= C.MARGIN).all()     # two shots: no solution
    else:
        assert m.valid[left].mean() > 0.9                                              # three of four remain
    assert np.array_equal(m.valid[~left], r.valid[~left]) and (~clear).sum() <= MAX_WITHOUT_MARGIN and banded.sum() >= 400


def masked_weights(n_lights, size=C.SIZE):
    """Shot 1 has weight 0 on the left half of the columns."""
    w = np.ones((n_lights,) + tuple(size), dtype=np.float32)
    w[1, :, :size[1] // 2] = 0.0
    return w


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("iterations", [1, 2, 3, 4])
def test_iterations_on_the_shadowed_set(iterations, size):
    r, r32 = solved("shadowed", size, iterations=iterations), solved("shadowed", size, dtype=np.float32, iterations=iterations)
    clear, _, banded = C.classes(r)
    err = float32_error(r32, r)
    print("shadowed %s K=%d: valid %d  margin < 1e-4: %d  banded %d  float32 oracle %.2e -> band %.0e  passes up to %d"
          % (size, iterations, int(r.valid.sum()), int((~clear).sum()), int(banded.sum()), err, band_for(err), int(r.passes.max())))
    want = ITERATIONS[(iterations, size[1])]
    assert (~clear).sum() <= MAX_WITHOUT_MARGIN and banded.sum() >= 800 and r.passes.max() == iterations
    assert np.array_equal(r32.valid[clear], r.valid[clear])
    assert err <= 1.25 * want and band_for(err) == band_for(want)
