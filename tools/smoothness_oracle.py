"""The smoothness prior of include/pbr_hip.h (pbr_smoothness_step; csrc/smoothness.hip) in numpy: the definition in float64, and the same
in float32 in the order the kernel's comment names -- the yardstick of tests/test_smoothness_host.py and tests/test_gpu_smoothness.py.

    value, grad = evaluate(p, lam, kind="charbonnier", eps=1e-3, wrap=False, weights=None, reduction="mean", dtype=np.float64)

`p` is [C,H,W] or [B,C,H,W]; `weights` None, [1,H,W] (shared by the batch) or [B,1,H,W].  The arithmetic runs on the values handed in:
pass what the device holds (a float16 tensor's values as they are), so that input rounding is part of no error.  `dtype=np.float32`:
every product, sum and difference is rounded to float32 on its own, in this order --
    s = 0; for c: s = (s + dx_c dx_c) + dy_c dy_c
    L2:           phi = s                   q = (k w) 2
    Charbonnier:  r = sqrt(s + eps eps)     phi = s / (r + eps)     q = (k w) / r
    g_c = (left + up) - (q dx_c + q dy_c),  left = (q dx_c)(y, x-1), up = (q dy_c)(y-1, x)
-- with k rounded once from float64; the value is the float64 sum of the float32 products w phi, times the float64 k (the kernel's
partial sums are float64 per lane and rounded to float32 once per workgroup).  The gradient is returned in `dtype`, unrounded to the
map's storage type: a float16 map's gradient is this, rounded once."""
import numpy as np

KINDS = ("l2", "charbonnier")


def scale(lam, shape, reduction):
    """k of the definition, float64: lambda / (B H W) for "mean", lambda for "sum"."""
    if reduction == "mean":
        b = shape[0] if len(shape) == 4 else 1
        return float(lam) / float(b * shape[-2] * shape[-1])
    if reduction == "sum":
        return float(lam)
    raise ValueError("reduction is 'mean' or 'sum', got %r" % (reduction,))


def _forward_difference(p, axis, wrap):
    """p(i + 1) - p(i) along `axis`; the last one wraps, or is exactly 0."""
    d = np.roll(p, -1, axis=axis) - p
    if not wrap:
        last = [slice(None)] * p.ndim
        last[axis] = -1
        d[tuple(last)] = 0
    return d


def _from_before(a, axis, wrap):
    """a(i - 1) along `axis`; the first one wraps, or is exactly 0."""
    out = np.roll(a, 1, axis=axis)
    if not wrap:
        first = [slice(None)] * a.ndim
        first[axis] = 0
        out[tuple(first)] = 0
    return out


def evaluate(p, lam, kind="charbonnier", eps=1e-3, wrap=False, weights=None, reduction="mean", dtype=np.float64):
    """(R, g): the value as a Python float, the gradient in p's shape."""
    if kind not in KINDS:
        raise ValueError("kind is one of %s, got %r" % (KINDS, kind))
    ft = np.dtype(dtype).type
    shape = tuple(np.shape(p))
    x = np.asarray(p, dtype=np.float64).astype(ft).reshape((-1,) + shape[-3:])                 # [B,C,H,W]
    B, C, H, W = x.shape
    if not 1 <= C <= 4:
        raise ValueError("1 to 4 channels, got %d" % C)
    k64 = scale(lam, shape, reduction)
    k = ft(k64)
    if weights is None:
        w = np.ones((B, 1, H, W), dtype=ft)
    else:
        w = np.broadcast_to(np.asarray(weights, dtype=np.float64).astype(ft).reshape((-1, 1, H, W)), (B, 1, H, W))
    dx, dy = _forward_difference(x, 3, wrap), _forward_difference(x, 2, wrap)
    s = np.zeros((B, 1, H, W), dtype=ft)
    for c in range(C):
        s = (s + dx[:, c:c + 1] * dx[:, c:c + 1]) + dy[:, c:c + 1] * dy[:, c:c + 1]
    kw = k * w
    if kind == "l2":
        phi, q = s, kw * ft(2.0)
    else:
        e = ft(eps)
        root = np.sqrt(s + e * e)
        phi, q = s / (root + e), kw / root
    value = k64 * float(np.sum((w * phi).astype(np.float64)))
    qdx, qdy = q * dx, q * dy
    g = (_from_before(qdx, 3, wrap) + _from_before(qdy, 2, wrap)) - (qdx + qdy)
    return value, g.reshape(shape)
