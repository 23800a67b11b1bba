"""The definition of photometric-stereo initialisation (include/pbr_hip.h, pbr_photometric_stereo) in numpy: test
infrastructure only, the product never imports it.  float64 by default; `dtype=np.float32` evaluates the same formulas in float32 (every
operation correctly rounded, which the kernel's hardware reciprocals and fused multiply-adds are not).

Pixel (y, x) at P = (xs[x], -ys[y], 0), xs, ys the float32 linspace(-s/2, s/2, .) of the render kernels:
  1. point: d = light_l - P, w_l = d / (|d| + 1e-7), a_l = 1 / (|d|^2 + 1e-7); directional: w_l = light_l / max(|light_l|, 1e-12), a_l = 1
  2. r_lc = lin(T_lc) / (I_lc a_l), y_l = (r_l0 + r_l1 + r_l2) / 3
  3. m = 1; pass k < K: u_l = weight_l m_l, shots with u_l == 0 skipped; A = sum u w w^T, b = sum u y w; t = tr A; c = det A / (t/3)^3 (0 when
     t <= 0); c < kappa: invalid.  g = adj(A) b / det A; |g| 0 or not finite, or g_z <= 0: invalid.  k < K - 1: m_l = [w_l . g > tau |g|]
  4. n = g / |g| | (0, 0, 1) and u_l = weight_l where invalid
  5. albedo_c = clamp(pi sum u s r_c / sum u s^2, 0, 1), s_l = max(w_l . n, 0); 0 where the denominator is 0
  6. confidence = c | 0 where invalid
"""
import collections

import numpy as np

Stereo = collections.namedtuple("Stereo", "normal albedo confidence valid margin g used passes")


def srgb_to_linear(x, dtype=np.float64):
    """pbr_srgb_to_linear's function: the input clamped to [0, 1] (utils/functions.py:28-47)."""
    f = dtype
    t = np.clip(np.asarray(x, dtype=f), f(0), f(1))
    return np.where(t <= f(0.04045), t / f(12.92), np.power((t + f(0.055)) / f(1.055), f(2.4))).astype(f)


def linear_to_srgb(x, dtype=np.float64):
    """pbr_linear_to_srgb's function on values in [0, 1] (utils/functions.py:50-66)."""
    f = dtype
    c = np.clip(np.asarray(x, dtype=f), f(0), f(1))
    with np.errstate(invalid="ignore"):
        hi = f(1.055) * np.power(c, f(1.0 / 2.4)) - f(0.055)
    return np.where(c <= f(0.0031308), c * f(12.92), hi).astype(f)


def linspace32(size, n):
    """torch.linspace(-size/2, size/2, n) as ATen's device kernel and the render kernels evaluate it, float32: two-ended, one fused
    multiply-add per element (exact product and sum in float64, rounded once)."""
    lo, hi = np.float32(-float(size) / 2), np.float32(float(size) / 2)
    if n == 1:
        return np.array([lo], dtype=np.float32)
    step = np.float32((hi - lo) / np.float32(n - 1))
    i = np.arange(n)
    low = i < (n >> 1)
    v = np.where(low, np.float64(step) * i + np.float64(lo), np.float64(hi) - np.float64(step) * (n - 1 - i))
    return v.astype(np.float32)


def geometry(light, size, light_type="point", light_size=None, dtype=np.float64, window=None):
    """-> (w [L,3,H,W], a [L,H,W]) in `dtype`: the unit vectors towards the lights and the attenuations of step 1.  `window`
    (y0, x0, H_total, W_total): `size` is the window [y0, y0 + H) x [x0, x0 + W) of a grid of H_total x W_total pixels (the y_offset /
    H_total of torch_oracle.cook_torrance, on both axes)."""
    f = dtype
    H, W = size
    y0, x0, H_total, W_total = (0, 0, H, W) if window is None else window
    light = np.asarray(light, dtype=np.float64).reshape(-1, 3)
    L = light.shape[0]
    if light_type == "directional":
        norm = np.maximum(np.sqrt((light ** 2).sum(axis=1, keepdims=True)), 1e-12)
        unit = (light / norm).astype(np.float32).astype(f)             # (the library normalises in double on the host and passes float32)
        return np.broadcast_to(unit[:, :, None, None], (L, 3, H, W)).copy(), np.ones((L, H, W), dtype=f)
    if light_type != "point":
        raise ValueError("light_type")
    s = light_size or 1.0
    xs, ys = linspace32(s, W_total).astype(f)[x0:x0 + W], linspace32(s, H_total).astype(f)[y0:y0 + H]
    P = np.stack([np.broadcast_to(xs[None, :], (H, W)), np.broadcast_to(-ys[:, None], (H, W)), np.zeros((H, W), dtype=f)])
    d = light.astype(np.float32).astype(f)[:, :, None, None] - P[None]
    dd = (d * d).sum(axis=1)
    dist = np.sqrt(dd)
    return (d / (dist + f(1e-7))[:, None]).astype(f), (f(1) / (dd + f(1e-7))).astype(f)


def photometric_stereo(targets, weights, light, light_intensity, light_type="point", light_size=None, targets_srgb=True, iterations=3,
                       shadow_cos=0.1, min_condition=1e-4, albedo_srgb=False, dtype=np.float64, window=None) -> Stereo:
    """targets [L,3,H,W]; weights [L,H,W], [H,W] or None; light [L,3]; light_intensity [3] or [L,3]; `window`: geometry()'s.  Returns arrays of `dtype`:
      normal (3,H,W), albedo (3,H,W), confidence (H,W)     steps 4 - 6
      valid (H,W) bool
      margin (H,W) float64   the smallest distance of any decision the pixel went through to its threshold: |w_l . g / |g| - tau| over the
                             shots with a non-zero weight and the passes that predict a mask, |c - kappa| / kappa and |g_z| / |g| over the
                             passes.  A pixel with margin >= eps is one whose decisions no rounding of that size can flip.
      g (3,H,W)              the last solution (0 where there is none)
      used (L,H,W) bool      u_l != 0 in step 5
      passes (H,W) int       solves the pixel went through"""
    f = dtype
    T = np.asarray(targets)
    L, _, H, W = T.shape
    K, tau, kappa = int(iterations), f(np.float32(shadow_cos)), f(np.float32(min_condition))
    if weights is None:
        wt = np.ones((L, H, W), dtype=f)
    else:
        wt = np.asarray(weights)
        wt = np.broadcast_to(wt.reshape((-1, H, W)), (L, H, W)).astype(f)
    inten = np.broadcast_to(np.asarray(light_intensity, dtype=np.float64).reshape(-1, 3), (L, 3)).astype(np.float32).astype(f)
    w, att = geometry(light, (H, W), light_type, light_size, dtype=f, window=window)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lin = srgb_to_linear(T, f) if targets_srgb else T.astype(f)
        r = (lin / (inten[:, :, None, None] * att[:, None])).astype(f)                              # [L,3,H,W]
        y = ((r[:, 0] + r[:, 1] + r[:, 2]) / f(3)).astype(f)                                        # [L,H,W]
        has = wt != 0
        mask = np.ones((L, H, W), dtype=bool)
        active = np.ones((H, W), dtype=bool)
        valid = np.ones((H, W), dtype=bool)
        g = np.zeros((3, H, W), dtype=f)
        conf = np.zeros((H, W), dtype=f)
        margin = np.full((H, W), np.inf)
        passes = np.zeros((H, W), dtype=np.int64)
        used = has.copy()
        for k in range(K):
            use = mask & has
            A = np.zeros((3, 3, H, W), dtype=f)
            b = np.zeros((3, H, W), dtype=f)
            for l in range(L):
                u = np.where(use[l], wt[l], f(0))
                yl = np.where(use[l], y[l], f(0))
                for i in range(3):
                    b[i] += np.where(use[l], u * yl * w[l, i], f(0))
                    for j in range(3):
                        A[i, j] += np.where(use[l], u * w[l, i] * w[l, j], f(0))
            t = A[0, 0] + A[1, 1] + A[2, 2]
            adj = np.empty_like(A)
            adj[0, 0] = A[1, 1] * A[2, 2] - A[1, 2] * A[1, 2]
            adj[0, 1] = adj[1, 0] = A[0, 2] * A[1, 2] - A[0, 1] * A[2, 2]
            adj[0, 2] = adj[2, 0] = A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]
            adj[1, 1] = A[0, 0] * A[2, 2] - A[0, 2] * A[0, 2]
            adj[1, 2] = adj[2, 1] = A[0, 1] * A[0, 2] - A[0, 0] * A[1, 2]
            adj[2, 2] = A[0, 0] * A[1, 1] - A[0, 1] * A[0, 1]
            det = A[0, 0] * adj[0, 0] + A[0, 1] * adj[0, 1] + A[0, 2] * adj[0, 2]
            t3 = t / f(3)
            c = np.where(t > 0, det / (t3 * t3 * t3), f(0)).astype(f)
            margin = np.where(active, np.minimum(margin, np.abs(c.astype(np.float64) - float(kappa)) / float(kappa)), margin)
            passes += active
            fail_c = active & (c < kappa)
            gk = np.stack([(adj[i, 0] * b[0] + adj[i, 1] * b[1] + adj[i, 2] * b[2]) / det for i in range(3)]).astype(f)
            norm = np.sqrt((gk * gk).sum(axis=0))
            solved = active & ~fail_c
            bad_g = solved & ~((norm > 0) & np.isfinite(norm) & (gk[2] > 0))
            ratio = np.where(norm > 0, np.abs(gk[2].astype(np.float64)) / norm.astype(np.float64), 0.0)
            margin = np.where(solved & np.isfinite(ratio), np.minimum(margin, ratio), margin)
            margin = np.where(solved & ~np.isfinite(norm), 0.0, margin)
            ok = solved & ~bad_g
            valid &= ~(fail_c | bad_g)
            g = np.where(ok, gk, g)
            conf = np.where(ok, c, conf)
            used = np.where(ok, use, used)
            active = ok
            if k < K - 1:
                cosl = (w * gk[None]).sum(axis=1) / norm                                            # [L,H,W]
                new = cosl > tau
                dist = np.where(has, np.abs(cosl.astype(np.float64) - float(tau)), np.inf).min(axis=0)
                margin = np.where(ok, np.minimum(margin, dist), margin)
                mask = np.where(ok, new, mask)
        used = np.where(valid, used, has)
        conf = np.where(valid, conf, f(0))
        norm = np.sqrt((g * g).sum(axis=0))
        n = np.where(valid, g / norm, np.array([0, 0, 1], dtype=f)[:, None, None]).astype(f)
        s = np.maximum((w * n[None]).sum(axis=1), f(0))                                             # [L,H,W]
        num = np.zeros((3, H, W), dtype=f)
        den = np.zeros((H, W), dtype=f)
        for l in range(L):
            den += np.where(used[l], wt[l] * s[l] * s[l], f(0))
            for ch in range(3):
                num[ch] += np.where(used[l], wt[l] * s[l] * r[l, ch], f(0))
        albedo = np.where(den == 0, f(0), np.clip(f(np.pi) * num / den, f(0), f(1))).astype(f)
        if albedo_srgb:
            albedo = linear_to_srgb(albedo, f)
    return Stereo(n, albedo, conf.astype(f), valid, margin, g, used, passes)
