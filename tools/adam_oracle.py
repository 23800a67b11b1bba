"""The definition of pypbr_amd.optim.MaterialAdam's step (csrc/adam.hip, pbr_adam_step), in numpy: the yardstick of tests/test_adam_host.py and
tests/test_gpu_adam.py.  float64 is the definition; float32 (`dtype=np.float32`) is the same sequence with every operation rounded to float32
-- numpy rounds each correctly -- which is what the kernel computes, and whose distance from float64 sets the tests' bands.

Per element, step count t >= 1:
    m <- m + (g - m) (1 - beta1)
    v <- beta2 v + ((1 - beta2) g) g
    a = lr / (1 - beta1^t)      c = 1 / sqrt(1 - beta2^t)          (float64, once per group and step, then rounded to the working type)
    delta = (a m) / (sqrt(v) c + eps)
    p <- p - delta
then the projection of p:
    None             nothing
    bounds=(lo, hi)  clamp(p, lo, hi); either may be None
    "unit"           [3,H,W] / [B,3,H,W]: z <- max(z, min_z) when min_z is given, then p / max(|p|, 1e-12) over the pixel's three channels
                     with |p| = sqrt(fma(z, z, fma(y, y, x x))): the products added with ONE rounding each, which is what torch's
                     F.normalize computes on the host (and one instruction each on the device)
An element whose delta is exactly 0 ("unit": all three of the pixel) keeps the bits of its parameter: neither clamped nor renormalised.
NaN and infinity propagate (the comparisons of clamp and max leave a NaN a NaN).
fp16 parameters (`half=True`, float32 arithmetic): the state holds a float32 master; the update and the projection run on the master and the
parameter is the master rounded to nearest even; an element that keeps its bits keeps the master's too.  No device, no torch."""
from fractions import Fraction

import numpy as np


def coefficients(lr, betas, eps, t, dtype=np.float64):
    """(a, c, 1 - beta1, beta2, 1 - beta2, eps): float64 first, then one rounding to `dtype`."""
    b1, b2 = float(betas[0]), float(betas[1])
    a = float(lr) / (1.0 - b1 ** float(t))
    c = 1.0 / np.sqrt(1.0 - b2 ** float(t))
    return tuple(dtype(x) for x in (a, c, 1.0 - b1, b2, 1.0 - b2, float(eps)))


def _clamp_lo(x, lo):
    return np.where(x < lo, lo, x)          # a NaN stays a NaN


def _clamp_hi(x, hi):
    return np.where(x > hi, hi, x)


def fma(a, b, c):
    """round(a b + c) with one rounding, element by element in exact rational arithmetic (numpy has no fused multiply-add; the sets this
    yardstick sees are small).  float32 goes through the correctly rounded float64 value: a second rounding that matters for about one
    value in 2^29.  Non-finite operands take the plain expression."""
    a, b, c = np.broadcast_arrays(a, b, c)
    out = np.empty(a.shape, dtype=np.float64)
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist(), c.reshape(-1).tolist())):
        if np.isfinite(x) and np.isfinite(y) and np.isfinite(z):
            flat[i] = float(Fraction(x) * Fraction(y) + Fraction(z))
        else:
            flat[i] = x * y + z
    return out.astype(a.dtype)


def project(p, project=None, bounds=None, min_z=None):
    """The projection alone, of every element (the zero-update rule is step()'s)."""
    dt = p.dtype.type
    if project == "unit":
        if p.ndim not in (3, 4) or p.shape[-3] != 3:
            raise ValueError('"unit" projects [3,H,W] / [B,3,H,W]')
        x, y, z = p[..., 0, :, :], p[..., 1, :, :], p[..., 2, :, :]
        if min_z is not None:
            z = _clamp_lo(z, dt(min_z))
        d = _clamp_lo(np.sqrt(fma(z, z, fma(y, y, x * x))), dt(1e-12))
        return np.stack([x / d, y / d, z / d], axis=-3)
    if project is not None:
        raise ValueError("project is None or 'unit'")
    if bounds is not None:
        lo, hi = bounds
        if lo is not None:
            p = _clamp_lo(p, dt(lo))
        if hi is not None:
            p = _clamp_hi(p, dt(hi))
    return p


def step(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, project_kind=None, bounds=None, min_z=None, dtype=np.float64, half=False):
    """One step from the state (p, g, m, v) at step count t (the count AFTER the increment: the first step is t = 1).
    Returns (p, m, v), and the master in front of them when `half`: (p as float16, master, m, v); then `p` going in is the master."""
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        p, g, m, v = (np.asarray(x, dtype=dtype) for x in (p, g, m, v))
        a, c, omb1, b2, omb2, e = coefficients(lr, betas, eps, t, dt)
        m = m + (g - m) * omb1
        v = b2 * v + (omb2 * g) * g
        delta = (a * m) / (np.sqrt(v) * c + e)
        moved = project(p - delta, project_kind, bounds, min_z)
        keep = delta == 0
        if project_kind == "unit":
            keep = np.broadcast_to(np.all(keep, axis=-3, keepdims=True), p.shape)
        out = np.where(keep, p, moved).astype(dtype)
    if half:
        return out.astype(np.float16), out, m, v
    return out, m, v
