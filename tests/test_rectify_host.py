"""Photograph rectification on the host side (no GPU): the numpy oracle of the definition (tools/rectify_oracle.py) equals torch's
grid_sample; homography_from_corners maps its corners; camera_positions recovers synthetic poses; the C ABI declares and exports
pbr_rectify_images (ABI still 9) and returns every caller-error code before any device work; and the populations the GPU tests run on
(tools/rectify_cases.py) hold what those tests need -- full, partial and zero coverage, both sides of a horizon, clipped taps.

Population counts, recorded from the oracle (24 x 36 grid = 864 pixels; full / partial / zero coverage at S = 1 | 2 | 4):
  inside    864 / 0 / 0 at every S
  overhang  731 / 41 / 92 | 707 / 82 / 75 | 695 / 103 / 66
  horizon   151 / 23 / 690 | 143 / 39 / 682 | 140 / 54 / 670
  clip      631 / 54 / 179 | 616 / 84 / 164 | 607 / 100 / 157
Share of the positive-coverage pixels with coverage >= 0.25, per RUN of the GPU test (the three geometric sets in one launch | the clip
run): 0.992 | 0.985 at S = 1, 0.985 | 0.964 at S = 2, 0.975 | 0.956 at S = 4.  (The horizon set alone has 0.983 / 0.962 / 0.907: few pixels
in front of the camera, many of them on the photograph's edge.)  Zero-coverage pixels without margin (a sub-sample within 0.01 source
pixels of a bound, or |d| < 1e-9): at most 1 per set and S, of 66 ... 690."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rectify_cases as C  # noqa: E402
import rectify_oracle as O  # noqa: E402

import abi_header  # noqa: E402
from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import capture  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402

IMG = C.photograph()
HOM = C.homographies()
H, W = C.SIZE
Hs, Ws = C.SOURCE_SHAPE[:2]


# ---------------------------------------------------------------- the oracle against torch
@pytest.mark.parametrize("name", ["inside", "overhang"])
def test_oracle_equals_grid_sample_with_zeros_padding(name):
    """S = 1: the premultiplied value is grid_sample(image / 255) and the coverage grid_sample(ones), bilinear, zeros padding,
    align_corners=False, in float64 on the CPU."""
    r = O.rectify(IMG, HOM[name], C.SIZE)
    m = HOM[name]
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = m[2, 0] * xs + m[2, 1] * ys + m[2, 2]
    U, V = (m[0, 0] * xs + m[0, 1] * ys + m[0, 2]) / d, (m[1, 0] * xs + m[1, 1] * ys + m[1, 2]) / d      # continuous source positions
    grid = torch.from_numpy(np.stack([2 * U / Ws - 1, 2 * V / Hs - 1], axis=-1))[None]
    image = torch.from_numpy(IMG).permute(2, 0, 1)[None].double() / 255
    kw = dict(mode="bilinear", padding_mode="zeros", align_corners=False)
    value = torch.nn.functional.grid_sample(image, grid, **kw)[0].numpy()
    cover = torch.nn.functional.grid_sample(torch.ones_like(image[:, :1]), grid, **kw)[0, 0].numpy()
    print("%s: |value - grid_sample| %.2e, |coverage - grid_sample| %.2e" % (name, np.abs(value - r.value).max(), np.abs(cover - r.coverage).max()))
    assert np.abs(value - r.value).max() <= 1e-12 and np.abs(cover - r.coverage).max() <= 1e-12
    assert r.targets.shape == (3, H, W) and r.coverage.shape == (H, W)
    pos = r.coverage > 0
    assert np.abs(r.targets * r.coverage - r.value)[:, pos].max() <= 1e-15 and (r.targets[:, ~pos] == 0).all()


def test_oracle_integer_translation_is_a_copy():
    m = np.array([[1.0, 0, 5], [0, 1.0, -3], [0, 0, 1.0]])
    r = O.rectify(IMG, m, C.SIZE)
    want = np.zeros((H, W, 3))
    want[3:] = IMG[:H - 3, 5:5 + W].astype(np.float64) / 255
    assert np.array_equal(r.targets, want.transpose(2, 0, 1))
    assert np.array_equal(r.coverage[3:], np.ones((H - 3, W))) and (r.coverage[:3] == 0).all()
    assert (r.margin[0] == 2).all() and (r.margin[2] == 0).all() and (r.dmin == 1).all()      # row 0 maps to v = -3, row 2 onto the bound v = -1


# ---------------------------------------------------------------- corners
def test_homography_from_corners_maps_the_four_corners():
    corners = np.array([C.CORNERS["inside"], C.CORNERS["overhang"]])
    M = capture.homography_from_corners(corners, C.SIZE)
    assert M.dtype == torch.float64 and tuple(M.shape) == (2, 3, 3) and (M[:, 2, 2] == 1).all()
    grid = np.array([[0.0, 0, 1], [W, 0, 1], [W, H, 1], [0, H, 1]])
    for l in range(2):
        p = grid @ M[l].numpy().T
        assert (p[:, 2] > 0).all()
        assert np.abs(p[:, :2] / p[:, 2:] - corners[l]).max() <= 1e-11
    one = capture.homography_from_corners(torch.tensor(C.CORNERS["inside"]), C.SIZE)          # [4,2] -> [1,3,3]
    assert tuple(one.shape) == (1, 3, 3) and np.abs(one[0].numpy() - M[0].numpy()).max() <= 1e-6          # (float32 corners)
    # the unit square of the grid onto itself is the identity
    eye = capture.homography_from_corners([(0, 0), (W, 0), (W, H), (0, H)], C.SIZE)[0].numpy()
    assert np.abs(eye - np.eye(3)).max() <= 1e-13


@pytest.mark.parametrize("bad", [
    [(0, 0), (10, 0), (20, 0), (0, 10)],            # three in a line
    [(0, 0), (10, 0), (10, 0), (0, 10)],            # two equal
    [(0, 0), (10, 10), (10, 0), (0, 10)],           # a bow tie: not convex
    [(0, 0), (10, 0), (2, 2), (0, 10)],             # concave
])
def test_degenerate_corners_raise(bad):
    with pytest.raises(ValueError):
        capture.homography_from_corners(bad, C.SIZE)


def test_corner_and_size_shapes_are_checked():
    with pytest.raises(ValueError):
        capture.homography_from_corners(np.zeros((3, 2)), C.SIZE)
    with pytest.raises(ValueError):
        capture.homography_from_corners(C.CORNERS["inside"], (0, 4))
    with pytest.raises(ValueError):
        capture.homography_from_corners(np.full((4, 2), np.nan), C.SIZE)


# ---------------------------------------------------------------- camera round trip
def _pose_homography(Cw, R, f, principal, size, light_size):
    """The homography a pinhole camera at Cw with rotation R (world -> camera) makes of the point light's grid."""
    Hh, Ww = size
    s = light_size or 1.0
    K = np.array([[f, 0, principal[0]], [0, f, principal[1]], [0, 0, 1.0]])
    t = -R @ Cw
    G = np.stack([R[:, 0], R[:, 1], t], axis=1)                                    # plane point (X, Y, 1), Z = 0 -> camera
    # continuous output pixel (px, py, 1) -> plane point: X = (px - 0.5) s / (W - 1) - s / 2, Y = s / 2 - (py - 0.5) s / (H - 1)
    Ainv = np.array([[s / (Ww - 1), 0, -0.5 * s / (Ww - 1) - s / 2], [0, -s / (Hh - 1), 0.5 * s / (Hh - 1) + s / 2], [0, 0, 1.0]])
    M = K @ G @ Ainv
    return M / M[2, 2]


def _look_at(Cw, target, roll):
    z = target - Cw
    z = z / np.linalg.norm(z)                                                      # the camera looks along + z
    x = np.cross(z, np.array([0.0, 1.0, 0.0]))                                     # y down in the image: x = z x up ... right-handed
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    x, y = c * x + s * y, -s * x + c * y
    return np.stack([x, y, z])                                                     # rows: world -> camera


@pytest.mark.parametrize("light_size", [None, 2.5])
def test_camera_positions_recovers_synthetic_poses(light_size):
    poses = [((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.0), ((0.3, -0.2, 0.4), (0.05, 0.02, 0.0), 0.2), ((-0.5, 0.4, 1.2), (-0.1, 0.1, 0.0), -0.7),
             ((0.15, 0.6, 0.8), (0.0, -0.05, 0.0), 1.3), ((-0.25, -0.35, 0.55), (0.1, 0.0, 0.0), 3.0)]
    size, source, f, principal = (48, 64), (3000, 4000), 3100.0, (2011.5, 1490.25)
    Ms, want = [], []
    for Cw, target, roll in poses:
        Cw = np.array(Cw)
        R = _look_at(Cw, np.array(target), roll)
        assert abs(np.linalg.det(R) - 1) < 1e-12
        Ms.append(_pose_homography(Cw, R, f, principal, size, light_size))
        want.append(Cw)
    got = capture.camera_positions(np.stack(Ms), size, source, f, principal=principal, light_size=light_size)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(poses), 3)
    err = np.abs(got.numpy() - np.array(want)).max()
    print("camera round trip (light_size %s): max |C - C'| = %.2e" % (light_size, err))
    assert err <= 1e-9
    # the scale and the sign of a homography mean nothing
    again = capture.camera_positions(-3.0 * np.stack(Ms), size, source, f, principal=principal, light_size=light_size)
    assert np.abs(again.numpy() - np.array(want)).max() <= 1e-9
    # the default principal point is the image centre
    Cw = np.array([0.1, 0.2, 0.9])
    M = _pose_homography(Cw, _look_at(Cw, np.zeros(3), 0.4), f, (2000.0, 1500.0), size, light_size)
    assert np.abs(capture.camera_positions(M, size, source, f, light_size=light_size)[0].numpy() - Cw).max() <= 1e-9


def test_camera_positions_feed_the_oracle_of_the_perspective_camera():
    """The frontal shot: the camera above the grid's centre sees the grid's corner pixels' CENTRES where surface_points puts them."""
    import camera_oracle
    size, f, source = (5, 7), 800.0, (600, 800)
    Cw = np.array([0.0, 0.0, 0.75])
    M = _pose_homography(Cw, np.diag([1.0, -1.0, -1.0]), f, (400.0, 300.0), size, None)
    P = camera_oracle.surface_points(*size).double().numpy()                       # (3, H, W)
    for (y, x) in ((0, 0), (4, 6), (2, 3)):
        p = M @ np.array([x + 0.5, y + 0.5, 1.0])
        cam = np.diag([1.0, -1.0, -1.0]) @ (P[:, y, x] - Cw)
        # (surface_points is float32, as upstream's linspace: half an ulp of 0.5, 3e-8, times f / distance)
        assert np.abs(p[:2] / p[2] - (f * cam[:2] / cam[2] + np.array([400.0, 300.0]))).max() <= 3e-8 * f / 0.75
    assert np.abs(capture.camera_positions(M, size, source, f)[0].numpy() - Cw).max() <= 1e-12


# ---------------------------------------------------------------- the ABI surface
def test_header_declares_and_library_exports_the_entry_point():
    raw = abi_header.RAW
    assert "#define PBR_MAX_RECTIFY_IMAGES 16" in raw and N.MAX_RECTIFY_IMAGES == 16
    assert N.ABI_VERSION == 9 and "#define PBR_HIP_ABI_VERSION 9" in raw
    lib = N.lib()
    assert lib.pbr_abi_version() == 9 and lib.pbr_rectify_images is not None
    assert F.rectify is capture.rectify and F.homography_from_corners is capture.homography_from_corners
    assert F.camera_positions is capture.camera_positions
    import pypbr_amd
    assert pypbr_amd.capture is capture


def test_rectify_images_caller_errors_come_back_without_a_device():
    """Every check runs before anything is launched: the device pointers are never dereferenced."""
    lib = N.lib()
    eye = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]

    def call(src=0x10000, n=1, hs=8, ws=8, si=192, sh=24, sw=3, sc=1, hom=eye, targets=0x80000, weights=0x90000, h=8, w=8, s=1, clip=0, lin=0):
        table = None if hom is None else (ctypes.c_double * len(hom))(*hom)
        return lib.pbr_rectify_images(src, n, hs, ws, si, sh, sw, sc, table, targets, weights, h, w, s, clip, lin, None)
    assert call(src=None) == N.ERR_NULL_MAP and call(hom=None) == N.ERR_NULL_MAP
    assert call(targets=None) == N.ERR_NULL_MAP and call(weights=None) == N.ERR_NULL_MAP
    assert call(n=0) == N.ERR_SHAPE and call(n=-1) == N.ERR_SHAPE and call(n=17, hom=eye * 17) == N.ERR_SHAPE
    assert call(hs=0) == N.ERR_SHAPE and call(ws=0) == N.ERR_SHAPE and call(h=0) == N.ERR_SHAPE and call(w=0) == N.ERR_SHAPE and call(h=-2) == N.ERR_SHAPE
    assert call(h=(1 << 30) + 1) == N.ERR_SHAPE and call(h=1 << 21, w=(1 << 20)) == N.ERR_SHAPE          # an extent > 2^30, H * W > 2^40
    assert call(s=0) == N.ERR_SHAPE and call(s=3) == N.ERR_SHAPE and call(s=8) == N.ERR_SHAPE and call(s=-1) == N.ERR_SHAPE
    assert call(clip=-1) == N.ERR_SHAPE and call(clip=256) == N.ERR_SHAPE
    assert call(si=-1) == N.ERR_SHAPE and call(sh=-1) == N.ERR_SHAPE and call(sw=-1) == N.ERR_SHAPE and call(sc=-1) == N.ERR_SHAPE
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in (0, 4, 8):
            assert call(hom=eye[:k] + [bad] + eye[k + 1:]) == N.ERR_SHAPE
        assert call(n=2, hom=eye + eye[:5] + [bad] + eye[6:]) == N.ERR_SHAPE        # the second image's matrix


def test_python_argument_errors_need_no_device():
    img = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    eye = torch.eye(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="uint8"):
        capture.rectify(img.float(), eye, (4, 4))
    with pytest.raises(ValueError, match="uint8"):
        capture.rectify([np.zeros((8, 8, 3), dtype=np.uint16)], eye, (4, 4))
    with pytest.raises(ValueError, match="one size"):
        capture.rectify([np.zeros((8, 8, 3), dtype=np.uint8), np.zeros((8, 9, 3), dtype=np.uint8)], eye, (4, 4))
    with pytest.raises(ValueError, match="homograph"):
        capture.rectify(img, torch.zeros(2, 2, 3), (4, 4))
    with pytest.raises(ValueError, match="homograph"):
        capture.rectify(img, torch.zeros(3, 3, 3), (4, 4))                          # three matrices for two images
    with pytest.raises(ValueError, match="homograph"):
        capture.rectify(img, torch.zeros(9), (4, 4))
    with pytest.raises(ValueError, match="finite"):
        capture.rectify(img, eye * float("nan"), (4, 4))
    with pytest.raises(ValueError):
        capture.rectify(img[..., :2], eye, (4, 4))                                  # two channels
    with pytest.raises(ValueError):
        capture.rectify(img, eye, (4, 4), supersample=3)
    with pytest.raises(ValueError):
        capture.rectify(img, eye, (4, 4), clip_level=0)
    with pytest.raises(ValueError):
        capture.rectify(img, eye, (4, 4), clip_level=256)
    with pytest.raises(ValueError):
        capture.rectify(img, eye, (0, 4))
    with pytest.raises(ValueError):
        capture.rectify(img, eye, (4, 4), device="cpu")
    with pytest.raises(ValueError):
        capture.rectify([], eye, (4, 4))
    if not torch.cuda.is_available():                                               # valid arguments: the product has no CPU path
        with pytest.raises(RuntimeError):
            capture.rectify(img, eye, (4, 4))


def test_pil_images_are_taken_as_their_own_samples():
    from PIL import Image
    rgb, rgba = Image.fromarray(IMG), Image.fromarray(np.concatenate([IMG, IMG[:, :, :1]], axis=2))
    assert rgba.mode == "RGBA"
    a = capture._as_samples([rgb, rgb])
    assert len(a) == 2 and a[0].dtype == np.uint8 and np.array_equal(a[0], IMG)
    b = capture._as_samples([rgba])
    assert b[0].shape == (Hs, Ws, 4) and np.array_equal(b[0][:, :, :3], IMG)
    grey = capture._as_samples([Image.fromarray(IMG[:, :, 0])])                     # other modes are converted to RGB
    assert grey[0].shape == (Hs, Ws, 3) and np.array_equal(grey[0][:, :, 1], IMG[:, :, 0])
    t = capture._as_samples(IMG)
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (1, Hs, Ws, 3)


# ---------------------------------------------------------------- the populations of the GPU tests
EXPECTED = {    # name -> S -> (full, partial, zero)
    "inside": {1: (864, 0, 0), 2: (864, 0, 0), 4: (864, 0, 0)},
    "overhang": {1: (731, 41, 92), 2: (707, 82, 75), 4: (695, 103, 66)},
    "horizon": {1: (151, 23, 690), 2: (143, 39, 682), 4: (140, 54, 670)},
    "clip": {1: (631, 54, 179), 2: (616, 84, 164), 4: (607, 100, 157)},
}


def _oracle(name, S):
    return O.rectify(IMG, HOM["inside" if name == "clip" else name], C.SIZE, supersample=S, clip_level=C.CLIP_LEVEL if name == "clip" else None)


@pytest.mark.parametrize("S", [1, 2, 4])
def test_populations_hold_every_class_the_gpu_tests_compare(S):
    assert IMG.shape == (40, 56, 3) and IMG.dtype == np.uint8 and C.SIZE == (24, 36)
    results = {name: _oracle(name, S) for name in EXPECTED}
    for name, r in results.items():
        full, partial, zero = (int(k.sum()) for k in C.classes(r.coverage))
        print("%s S=%d: full %d partial %d zero %d" % (name, S, full, partial, zero))
        assert (full, partial, zero) == EXPECTED[name][S], name
        assert full + partial + zero == H * W and r.coverage.max() <= 1 + 1e-12
        if name == "inside":
            assert full == H * W
        else:
            assert min(full, partial, zero) >= 20, name
        # the exact-zero assertion of the GPU test skips the zero-coverage pixels without margin: fewer than 2 % of them
        unclear = int(((r.coverage == 0) & ~C.clear_zero(r)).sum())
        print("   zero-coverage pixels without margin: %d of %d" % (unclear, zero))
        assert unclear <= 1 and (zero == 0 or unclear < 0.02 * zero), name
    # the horizon: at least 50 pixels wholly in front of the camera and 50 wholly behind it
    m = HOM["horizon"]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    corners_d = np.stack([m[2, 0] * (xs + a) + m[2, 1] * (ys + b) + m[2, 2] for a in (0, 1) for b in (0, 1)])
    front, behind = int((corners_d.min(0) > 0).sum()), int((corners_d.max(0) < 0).sum())
    print("horizon: %d pixels in front, %d behind" % (front, behind))
    assert front >= 50 and behind >= 50
    mid = m[2, 0] * 20.0 + m[2, 1] * (H / 2.0) + m[2, 2]
    assert abs(mid) < 1e-15                                                         # d changes sign at X = 20 on the middle row
    assert (results["horizon"].coverage[:, 21:] == 0).all()
    # targets are compared directly where coverage >= 0.25: at least 95 % of the positive-coverage pixels of each run of the GPU test
    for run in (("inside", "overhang", "horizon"), ("clip",)):
        cov = np.concatenate([results[n].coverage.reshape(-1) for n in run])
        share = float((cov[cov > 0] >= 0.25).mean())
        print("run %s S=%d: %.4f of the positive-coverage pixels have coverage >= 0.25" % ("+".join(run), S, share))
        assert share >= 0.95, run


def test_clip_level_is_an_exact_integer_comparison_on_any_channel():
    img = np.full((4, 4, 3), 10, dtype=np.uint8)
    img[1, 1] = (10, 200, 10)                                                       # one channel at the level
    img[2, 2] = (199, 199, 199)                                                     # just below it
    eye = np.eye(3)
    r = O.rectify(img, eye, (4, 4), clip_level=200)
    assert r.coverage[1, 1] == 0 and (r.targets[:, 1, 1] == 0).all() and r.coverage[2, 2] == 1 and r.coverage.sum() == 15
    assert O.rectify(img, eye, (4, 4)).coverage.sum() == 16


def test_to_linear_goes_through_the_srgb_curve_before_weighting():
    m = np.array([[1.0, 0, 0.5], [0, 1.0, 0], [0, 0, 1.0]])                          # half a pixel: two taps of 0.5
    img = np.zeros((1, 3, 3), dtype=np.uint8)
    img[0, 0], img[0, 1] = 255, 0
    r = O.rectify(img, m, (1, 1), to_linear=True)
    assert abs(r.targets[0, 0, 0] - 0.5) < 1e-15                                    # the mean of srgb_to_linear(1) and srgb_to_linear(0), not srgb_to_linear(0.5)
    want = O.srgb_to_linear(np.arange(256) / 255.0)
    got = torch.from_numpy(np.arange(256) / 255.0)
    ref = torch.where(got <= 0.04045, got / 12.92, ((got + 0.055) / 1.055) ** 2.4).numpy()
    assert np.abs(want - ref).max() <= 1e-15
