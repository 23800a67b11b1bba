"""The populations the rectification tests run on (tests/test_rectify_host.py pins their make-up with the oracle alone, tests/test_gpu_rectify.py
runs the kernel on them): a 40 x 56 x 3 random uint8 photograph warped to a 24 x 36 grid by

  inside     the grid lies inside the photograph: every pixel fully covered
  overhang   the grid hangs over all four edges: full, partial and zero coverage
  horizon    overhang with m20 set so that d changes sign at X = 20 on the middle row: the grid's right part lies behind the camera
  clip       inside, with clip_level = 200: taps on bright samples count as uncovered

Test infrastructure only."""
import numpy as np

from pypbr_amd import capture

SOURCE_SHAPE = (40, 56, 3)           # (Hs, Ws, C)
SIZE = (24, 36)                      # (H, W)
CLIP_LEVEL = 200
CORNERS = {                          # source (u, v) of the grid's TL, TR, BR, BL corners
    "inside": [(8.3, 6.1), (47.2, 9.4), (44.9, 33.3), (5.6, 30.2)],
    "overhang": [(-6.5, 4.2), (50.1, -5.3), (61.7, 35.8), (3.3, 44.9)],
}
FULL = 1.0 - 1e-9                    # coverage from here up is "full": the four weights of a tap sum to 1 within a few ulp in float64
# A pixel whose every inside / outside decision is clear of rounding: no sub-sample within MARGIN source pixels of one of the four bounds, no |d| below DMIN.
MARGIN, DMIN = 0.01, 1e-9


HIGHLIGHTS = ((12, 26, 20, 36),)        # (row0, row1, col0, col1): patches of clipped samples inside `inside`


def photograph(seed: int = 20240) -> np.ndarray:
    """Random samples below CLIP_LEVEL with a patch of random samples from CLIP_LEVEL up (flash highlights): with independent
    samples over the whole range next to no pixel would have all of its taps clipped, or none of them."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, CLIP_LEVEL, SOURCE_SHAPE, dtype=np.uint8)
    for r0, r1, c0, c1 in HIGHLIGHTS:
        img[r0:r1, c0:c1] = rng.integers(CLIP_LEVEL, 256, (r1 - r0, c1 - c0, SOURCE_SHAPE[2]), dtype=np.uint8)
    return img


def homographies() -> dict:
    """name -> float64 3x3."""
    H, _ = SIZE
    m = {k: capture.homography_from_corners(np.array(v), SIZE)[0].numpy() for k, v in CORNERS.items()}
    hz = m["overhang"].copy()
    hz[2, 0] = -(hz[2, 1] * (H / 2.0) + hz[2, 2]) / 20.0
    m["horizon"] = hz
    return m


def classes(coverage: np.ndarray):
    """(full, partial, zero) boolean masks of a coverage array."""
    return coverage >= FULL, (coverage > 0) & (coverage < FULL), coverage == 0


def clear_zero(r) -> np.ndarray:
    """Where an oracle result (tools/rectify_oracle.Rectified) has zero coverage with margin: the kernel must write exact zeros there."""
    return (r.coverage == 0) & (r.margin >= MARGIN) & (r.dmin >= DMIN)
