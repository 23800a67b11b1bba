"""The populations the photometric-stereo tests run on (tests/test_photometric_host.py pins their make-up with the oracle alone,
tests/test_gpu_photometric.py runs the kernel on them): a 24 x 36 grid -- ragged against the kernel's 16 x 16-lane tile on both axes, in
the quad form and in the pixel form -- and its 24 x 35 sibling (the pixel form only), light_size 1, L = 8 point lights on a circle of
radius 0.7 (`n_lights`: the same sets under 3, 4 or 16 lights on that circle).

  gentle     normals of the height field with slopes hx = 0.6 sin(7x + 1) cos(5y), hy = 0.6 cos(6y) sin(4x + 2), n = normalize(-hx, -hy, 1);
             lights at heights 0.6 / 0.8 alternating; albedo uniform in [0.15, 0.9]; exactly Lambertian targets, sRGB-encoded
  shadowed   the same with slope amplitudes 1.2 and heights 0.3 / 0.45: about a fifth of the observations in attached shadow
  partial    gentle, shot l's weight zero on the columns left of W (l + 1) / (L + 2): a pixel sees 0 ... 8 shots
  rendered   the gentle maps as a rough dielectric (roughness 0.6, metallic 0) through the Cook-Torrance model, sRGB targets: made by
             F.cook_torrance_stack on the device, and by the committed torch oracle on the host

Test infrastructure only."""
import collections

import numpy as np

import photometric_oracle as O

SIZE = (24, 36)
SIBLING = (24, 35)
N_LIGHTS = 8
RADIUS = 0.7
LIGHT_SIZE = 1.0
SETS = {                                # name -> (slope amplitude, (even, odd) light heights, intensity of every channel)
    "gentle": (0.6, (0.6, 0.8), 1.2),
    "shadowed": (1.2, (0.3, 0.45), 0.25),
}
ROUGHNESS = 0.6
MARGIN = 1e-4                           # a pixel with at least this margin keeps its decisions under float32 rounding
WELL_CONDITIONED = 0.05                 # the banded comparison is made where the oracle's confidence is at least this

Case = collections.namedtuple("Case", "targets weights light intensity normal albedo shadowed")


def lights(heights, n_lights=N_LIGHTS) -> np.ndarray:
    hop = 3 if n_lights % 3 else 1                                                     # (a count 3 divides: three places on would come back to the start)
    ang = 2.0 * np.pi * ((hop * np.arange(n_lights)) % n_lights + 0.25) / n_lights    # shot l hops three places on: any three consecutive shots span the circle
    z = np.where(np.arange(n_lights) % 2 == 0, heights[0], heights[1])
    return np.stack([RADIUS * np.cos(ang), RADIUS * np.sin(ang), z], axis=1).astype(np.float32).astype(np.float64)


def normals(amplitude, size=SIZE) -> np.ndarray:
    """(3, H, W) float64 unit normals on the point light's grid."""
    H, W = size
    xs, ys = O.linspace32(LIGHT_SIZE, W).astype(np.float64), O.linspace32(LIGHT_SIZE, H).astype(np.float64)
    x, y = np.meshgrid(xs, -ys, indexing="xy")
    hx = amplitude * np.sin(7 * x + 1) * np.cos(5 * y)
    hy = amplitude * np.cos(6 * y) * np.sin(4 * x + 2)
    n = np.stack([-hx, -hy, np.ones_like(hx)])
    return n / np.sqrt((n * n).sum(axis=0))


def albedo(size=SIZE, seed=31) -> np.ndarray:
    return np.random.default_rng(seed).uniform(0.15, 0.9, (3,) + tuple(size))


def partial_weights(size=SIZE, n_lights=N_LIGHTS) -> np.ndarray:
    H, W = size
    cols = np.arange(W)[None, None, :]
    first = (W * (np.arange(n_lights) + 1.0) / (n_lights + 2))[:, None, None]
    return np.broadcast_to((cols >= first).astype(np.float32), (n_lights, H, W)).copy()


def lambertian(name, size=SIZE, encode=True, n_lights=N_LIGHTS) -> Case:
    """`gentle`, `shadowed` or `partial`.  targets: float32 sRGB-encoded (encode) or float64 linear; `shadowed` [L,H,W] marks the
    observations in attached shadow (n . w_l <= 0).  `n_lights`: another count of lights on the same circle (1 ... 16)."""
    amplitude, heights, inten = SETS["gentle" if name == "partial" else name]
    inten = float(np.float32(inten))                                                # (lights and intensities travel as float32)
    n, rho, pos = normals(amplitude, size), albedo(size), lights(heights, n_lights)
    w, att = O.geometry(pos, size, "point", LIGHT_SIZE)
    cos = (w * n[None]).sum(axis=1)                                                  # [L,H,W]
    lin = rho[None] / np.pi * inten * (np.maximum(cos, 0.0) * att)[:, None]         # [L,3,H,W]
    assert lin.max() < 1.0, lin.max()                                                # nothing clipped: the data stay exactly Lambertian
    targets = O.linear_to_srgb(lin).astype(np.float32) if encode else lin
    weights = partial_weights(size, n_lights) if name == "partial" else None
    return Case(targets, weights, pos, np.full(3, inten), n, rho, cos <= 0)


def classes(r, margin=MARGIN, well=WELL_CONDITIONED):
    """Boolean masks of an oracle result: (clear, invalid with margin, banded) -- `clear`: every decision has the margin; `banded`: valid,
    clear and well conditioned."""
    clear = r.margin >= margin
    return clear, clear & ~r.valid, clear & r.valid & (r.confidence >= well)
