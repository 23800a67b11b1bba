"""The definition of photograph rectification (include/pbr_hip.h, pbr_rectify_images) in numpy float64: test
infrastructure only, the product never imports it.

Output pixel (y, x), S = supersample, sub-samples i, j < S:
  1. X = x + (i + 0.5) / S, Y = y + (j + 0.5) / S                         (output pixel centres at + 0.5)
  2. d = m20 X + m21 Y + m22, u = (m00 X + m01 Y + m02) / d - 0.5, v = (m10 X + m11 Y + m12) / d - 0.5      (source index units)
  3. outside when d <= 0, u or v not finite, u <= -1, u >= Ws, v <= -1 or v >= Hs
  4. else bilinear taps at (floor u, floor v) and its three neighbours; a tap outside the image, or (clip_level = k) with any of its three
     samples >= k, contributes 0 to the value and 0 to the coverage
  value_c = sum w_t sample_tc / 255 / S^2, coverage = sum w_t / S^2 (to_linear: sample / 255 through srgb_to_linear first),
  targets_c = clamp(value_c / coverage, 0, 1) where coverage > 0, 0 where coverage == 0.
"""
import collections

import numpy as np

Rectified = collections.namedtuple("Rectified", "targets coverage value margin dmin")


def srgb_to_linear(x):
    """utils/functions.py:28-47 on values in [0, 1], float64."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def rectify(image, homography, size, supersample=1, clip_level=None, to_linear=False) -> Rectified:
    """image: uint8 (Hs, Ws, C >= 3), channels 0..2 are read; homography: 3x3; size: (H, W).  Returns float64 arrays:
      targets  (3, H, W)   clamp(value / coverage, 0, 1), 0 where coverage == 0
      coverage (H, W)      the weights
      value    (3, H, W)   the premultiplied value, = weights * targets before the clamp
      margin   (H, W)      the smallest distance, in source pixels, of any sub-sample with d > 0 from one of step 3's four bounds
      dmin     (H, W)      the smallest |d| of any sub-sample
    A pixel with margin >= eps and dmin >= eps' is one whose inside / outside decisions no rounding of the coordinates can flip."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] < 3:
        raise ValueError("image must be uint8 (Hs, Ws, C >= 3)")
    S = int(supersample)
    if S not in (1, 2, 4):
        raise ValueError("supersample must be 1, 2 or 4")
    Hs, Ws = image.shape[:2]
    H, W = size
    m = np.asarray(homography, dtype=np.float64).reshape(3, 3)
    samples = image[:, :, :3].astype(np.int64)
    unit = samples.astype(np.float64) / 255.0
    if to_linear:
        unit = srgb_to_linear(unit)
    live_sample = np.ones((Hs, Ws), dtype=bool) if not clip_level else (samples.max(axis=2) < int(clip_level))

    value, coverage = np.zeros((3, H, W)), np.zeros((H, W))
    margin, dmin = np.full((H, W), np.inf), np.full((H, W), np.inf)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(S):
            for i in range(S):
                X, Y = xs + (i + 0.5) / S, ys + (j + 0.5) / S
                d = m[2, 0] * X + m[2, 1] * Y + m[2, 2]
                u = (m[0, 0] * X + m[0, 1] * Y + m[0, 2]) / d - 0.5
                v = (m[1, 0] * X + m[1, 1] * Y + m[1, 2]) / d - 0.5
                front = (d > 0) & np.isfinite(u) & np.isfinite(v)
                inside = front & (u > -1) & (u < Ws) & (v > -1) & (v < Hs)
                dist = np.minimum(np.minimum(np.abs(u + 1), np.abs(u - Ws)), np.minimum(np.abs(v + 1), np.abs(v - Hs)))
                margin = np.minimum(margin, np.where(front, dist, np.inf))
                dmin = np.minimum(dmin, np.abs(d))
                us, vs = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
                x0, y0 = np.floor(us), np.floor(vs)
                fx, fy = us - x0, vs - y0
                x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
                for ty, wy in ((0, 1.0 - fy), (1, fy)):
                    for tx, wx in ((0, 1.0 - fx), (1, fx)):
                        xi, yi = x0 + tx, y0 + ty
                        ok = inside & (xi >= 0) & (xi < Ws) & (yi >= 0) & (yi < Hs)
                        xc, yc = np.clip(xi, 0, Ws - 1), np.clip(yi, 0, Hs - 1)
                        ok &= live_sample[yc, xc]
                        w = np.where(ok, wx * wy, 0.0)
                        coverage += w
                        value += w[None] * np.moveaxis(unit[yc, xc], -1, 0)
    value /= S * S
    coverage /= S * S
    with np.errstate(divide="ignore", invalid="ignore"):
        targets = np.where(coverage > 0, np.clip(value / coverage, 0.0, 1.0), 0.0)
    return Rectified(targets, coverage, value, margin, dmin)
