"""From photographs to what a light-stack fit takes: the first step of photograph -> rectify -> fit -> save.  No upstream counterpart.

  homography_from_corners   four clicked corners per shot -> the 3x3 homography of that shot          (host, float64)
  rectify                   photographs as uint8 (H,W,C) samples + homographies -> targets [L,3,H,W] and coverage weights [L,1,H,W]
                            on the texture grid, ONE kernel pass (csrc/rectify.hip, pbr_rectify_images)
  camera_positions          homographies + a focal length -> where each shot was taken from, the [L,3] `view_dir` of view_type="point"
                                                                                                        (host, float64)
  photometric_stereo        targets, weights and the lights of the shots -> the normal, albedo and confidence a fit STARTS from: a
                            Lambertian least-squares solve per pixel, re-solved with the predicted attached shadows masked out, ONE kernel
                            pass (csrc/photometric.hip, pbr_photometric_stereo)
  initial_material          ... as a BasecolorMetallicMaterial with a constant roughness and metallic 0

The conventions (include/pbr_hip.h, pbr_rectify_images, is the definition; tools/rectify_oracle.py restates it in numpy float64):
output pixel (y, x) has its centre at (x + 0.5, y + 0.5), so the grid spans [0, W] x [0, H]; a homography M maps such a continuous grid
position to a continuous source position (U, V) = M (X, Y, 1), source pixel centres at + 0.5 too; samples are taken with bilinear taps
and zeros padding, exactly F.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False); `weights` is the coverage -- the
taps' weights that landed inside the photograph on unclipped samples -- and `targets` the covered taps' mean, 0 where nothing is covered.
There is no threshold: a caller who wants a binary mask thresholds `weights`.

None of this is differentiable: the photographs are data.  A gradient with respect to the homography (alignment refinement) or the image is
out of scope."""
import ctypes
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N
from . import _upload as U
from ._dispatch import launch

# calls since import: pbr_rectify_images (one per chunk of N.MAX_RECTIFY_IMAGES photographs), pbr_photometric_stereo (one per call)
CALLS = {"rectify_images": 0, "photometric_stereo": 0}


def _size(size, what: str) -> Tuple[int, int]:
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("%s: a size is (height, width), got %r" % (what, size)) from None
    if H < 1 or W < 1:
        raise ValueError("%s: a size is (height, width) with both >= 1, got %r" % (what, size))
    return H, W


def _homographies(h, n: Optional[int], what: str) -> np.ndarray:
    """-> float64 [L,3,3] on the host; [3,3] is one shot (or, with n shots, the same matrix for each)."""
    m = h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)
    if m.dtype.kind not in "fiu" or m.ndim not in (2, 3) or m.shape[-2:] != (3, 3):
        raise ValueError("%s: homographies must be [L,3,3] or [3,3], got %s" % (what, m.shape))
    m = np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 3, 3)
    if n is not None and m.shape[0] != n:
        if m.shape[0] != 1:
            raise ValueError("%s: %d homographies for %d images" % (what, m.shape[0], n))
        m = np.ascontiguousarray(np.broadcast_to(m, (n, 3, 3)))
    if not np.isfinite(m).all():
        raise ValueError("%s: a homography entry is not finite" % what)
    return m


def homography_from_corners(corners, size) -> torch.Tensor:
    """corners [L,4,2] or [4,2]: the source-pixel (u, v) positions of the grid's OUTER corners in the order TL, TR, BR, BL -- continuous
    positions, pixel centres at + 0.5, so (0, 0) is the top-left corner of the top-left pixel.  They are where (0, 0), (W, 0), (W, H) and
    (0, H) of the H x W grid (`size`) land.  Returns the homographies, float64 [L,3,3] with m22 = 1, from an 8x8 solve per shot on the host.
    Degenerate corners (three of them in a line, two equal, or a quadrilateral that is not convex, whose horizon would cross the grid)
    raise ValueError."""
    H, W = _size(size, "homography_from_corners")
    c = corners.detach().cpu().numpy() if isinstance(corners, torch.Tensor) else np.asarray(corners)
    if c.ndim not in (2, 3) or c.shape[-2:] != (4, 2) or c.dtype.kind not in "fiu":
        raise ValueError("homography_from_corners: corners must be [L,4,2] or [4,2], got %s" % (c.shape,))
    c = c.astype(np.float64).reshape(-1, 4, 2)
    if not np.isfinite(c).all():
        raise ValueError("homography_from_corners: a corner is not finite")
    grid = np.array([[0.0, 0.0], [W, 0.0], [W, H], [0.0, H]])
    out = np.empty((c.shape[0], 3, 3))
    for l, quad in enumerate(c):
        A, b = np.zeros((8, 8)), np.zeros(8)
        for k, ((X, Y), (u, v)) in enumerate(zip(grid, quad)):
            A[2 * k] = [X, Y, 1, 0, 0, 0, -u * X, -u * Y]
            A[2 * k + 1] = [0, 0, 0, X, Y, 1, -v * X, -v * Y]
            b[2 * k], b[2 * k + 1] = u, v
        # columns scaled to unit size first: the condition number then speaks about the corners, not about W and H
        scale = np.abs(A).max(axis=0)
        if (scale == 0).any() or np.linalg.cond(A / scale) > 1e12:
            raise ValueError("homography_from_corners: the corners of shot %d are degenerate: %s" % (l, quad.tolist()))
        m = np.append(np.linalg.solve(A / scale, b) / scale, 1.0).reshape(3, 3)
        if not np.isfinite(m).all() or ((grid @ m[2, :2]) + 1.0 <= 1e-12).any():
            raise ValueError("homography_from_corners: the corners of shot %d are not a convex quadrilateral: %s" % (l, quad.tolist()))
        out[l] = m
    return torch.from_numpy(out)


def _as_samples(images) -> Union[torch.Tensor, list]:
    """images -> a uint8 [L,Hs,Ws,C] tensor (device or host), or a list of equal-sized (Hs,Ws,C) numpy arrays.  Raises ValueError."""
    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8:
            raise ValueError("rectify: photographs are uint8 samples, got %s (16-bit and float photographs are not supported)" % images.dtype)
        t = images.unsqueeze(0) if images.dim() == 3 else images
        if t.dim() != 4 or t.shape[-1] not in (3, 4) or min(t.shape) < 1:
            raise ValueError("rectify: images must be [L,Hs,Ws,C] or [Hs,Ws,C] with C 3 or 4, got %s" % (tuple(images.shape),))
        return t
    if isinstance(images, np.ndarray):
        return _as_samples(torch.from_numpy(images))
    if not isinstance(images, (list, tuple)) or not images:
        raise ValueError("rectify: images must be a uint8 tensor or a list of PIL images / numpy arrays")
    arrays = []
    for im in images:
        if isinstance(im, torch.Tensor):
            im = im.detach().cpu().numpy()
        elif not isinstance(im, np.ndarray):               # a PIL image: its own samples, RGB or RGBA as they are
            if getattr(im, "mode", None) not in ("RGB", "RGBA"):
                im = im.convert("RGB")
            im = np.asarray(im)
        if im.dtype != np.uint8:
            raise ValueError("rectify: photographs are uint8 samples, got %s" % im.dtype)
        if im.ndim != 3 or im.shape[2] not in (3, 4) or min(im.shape) < 1:
            raise ValueError("rectify: an image must be (Hs,Ws,C) with C 3 or 4, got %s" % (im.shape,))
        arrays.append(np.ascontiguousarray(im))
    if any(a.shape != arrays[0].shape for a in arrays):
        raise ValueError("rectify: the images of one call share one size, got %s" % sorted({a.shape for a in arrays}))
    return arrays


def _upload_samples(samples, device: torch.device) -> torch.Tensor:
    """Host samples -> a dense uint8 [L,Hs,Ws,C] device tensor: the bytes as they are, through _upload's page-locked stage, ONE transfer."""
    if isinstance(samples, torch.Tensor):
        shape = tuple(samples.shape)
        host, slot = U._upload_stage(samples.numel())
        U._stage_copy(host, samples.contiguous(), samples.numel())
    else:                                                  # (numpy arrays, PIL's read-only ones among them: copied array to array)
        shape = (len(samples),) + samples[0].shape
        host, slot = U._upload_stage(len(samples) * samples[0].size)
        np.stack(samples, out=host.numpy().reshape(shape))
    total = host.numel()
    dev = torch.empty(total, dtype=torch.uint8, device=device)
    dev.copy_(host, non_blocking=True)
    if slot is not None:
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(device))
    return dev.view(shape)


def rectify(images, homographies, size, *, supersample: int = 1, clip_level: Optional[int] = None, to_linear: bool = False,
            device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Photographs -> (targets [L,3,H,W], weights [L,1,H,W]), float32 on the device, in one pass of csrc/rectify.hip.

    images         a uint8 tensor [L,Hs,Ws,C] or [Hs,Ws,C], C 3 or 4 (only R, G, B are read), on the device or the host; or a list of
                   equal-sized PIL images / numpy arrays.  Host data goes up as BYTES (a quarter of a float upload) through the page-locked
                   stage of _upload; a device tensor is read through its own strides, so an RGBA tensor or a crop travels as it is.
    homographies   [L,3,3] or [3,3] (homography_from_corners): continuous grid position (X, Y, 1) -> continuous source position.
    size           (H, W) of the texture grid.
    supersample    1, 2 or 4: S x S sub-samples per output pixel, averaged.
    clip_level     k in 1..255: a tap with any of R, G, B >= k (a clipped flash highlight) counts as uncovered; None: off.
    to_linear      every tap's sample / 255 goes through srgb_to_linear before it is weighted.
    device         where the work runs: the images' device if they are on one, else the current ROCm device.

    weights is the coverage in [0, 1]; targets is clamp(value / coverage, 0, 1) and exactly 0 where nothing is covered (always finite).
    Both go unchanged into functional.rendering_loss_mse_stack(targets=, weights=) and MultiLightRenderingLoss.  More than 16 images are
    served in chunks of 16.  Not differentiable.  ValueError (non-uint8 samples, unequal sizes, a homography that is not [L,3,3] or
    [3,3], a bad option) is raised before any device work."""
    H, W = _size(size, "rectify")
    samples = _as_samples(images)
    L = samples.shape[0] if isinstance(samples, torch.Tensor) else len(samples)
    m = _homographies(homographies, L, "rectify")
    if supersample not in (1, 2, 4):
        raise ValueError("rectify: supersample must be 1, 2 or 4, got %r" % (supersample,))
    clip = 0 if clip_level is None else int(clip_level)
    if clip_level is not None and not 1 <= clip <= 255:
        raise ValueError("rectify: clip_level must be in 1..255 or None, got %r" % (clip_level,))
    on_device = isinstance(samples, torch.Tensor) and samples.is_cuda
    if device is None:
        dev = samples.device if on_device else None
    else:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("rectify: the work runs on a ROCm device, got device=%s" % (device,))
    N.require_device()
    if dev is None or dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if on_device:
        src = samples.to(dev)
        if any(s < 0 for s in src.stride()):
            src = src.contiguous()
    else:
        src = _upload_samples(samples, dev)
    Hs, Ws = src.shape[1], src.shape[2]
    targets = torch.empty((L, 3, H, W), dtype=torch.float32, device=dev)
    weights = torch.empty((L, 1, H, W), dtype=torch.float32, device=dev)
    fn, plane = N.lib().pbr_rectify_images, H * W
    for l0 in range(0, L, N.MAX_RECTIFY_IMAGES):
        n = min(N.MAX_RECTIFY_IMAGES, L - l0)
        table = (ctypes.c_double * (9 * n))(*m[l0:l0 + n].reshape(-1).tolist())
        launch(dev, fn, src.data_ptr() + l0 * src.stride(0), n, Hs, Ws, src.stride(0), src.stride(1), src.stride(2), src.stride(3), table,
               targets.data_ptr() + 4 * 3 * plane * l0, weights.data_ptr() + 4 * plane * l0, H, W, int(supersample), clip, 1 if to_linear else 0)
        CALLS["rectify_images"] += 1
    return targets, weights


def camera_positions(homographies, size, source_size, focal_px: float, principal: Optional[Sequence[float]] = None,
                     light_size: Optional[float] = None) -> torch.Tensor:
    """Where each photograph was taken from, in the point light's coordinates: float64 [L,3], what view_type="point" takes as a [L,3]
    `view_dir` (`.float()` and `.to(device)` it).  Host-only float64 linear algebra, a planar pose from a homography:

      G = K^-1 M A    K = [[f, 0, cx], [0, f, cy], [0, 0, 1]] with f = `focal_px` and (cx, cy) = `principal`, in continuous source pixels (default:
                      the image centre (Ws / 2, Hs / 2) of `source_size` = (Hs, Ws)); A maps the plane point (X, Y, 1) of the grid
                      P = (xs[x], -ys[y], 0) -- linspace(-s/2, s/2, .) per axis, s = light_size or 1.0, the point light's grid -- to the continuous
                      output pixel (index + 0.5) that M starts from;
      G is scaled so that the mean norm of its first two columns is 1, its sign chosen so that G[2,2] > 0 (the plane in front of the camera);
      R = [g0, g1, g0 x g1] projected onto the rotations by SVD;  C = -R^T g2.

    The camera looks along its +z with y down (image rows), the plane has y up and its normal +z towards the camera: for a frontal shot
    R = diag(1, -1, -1) and C = (0, 0, distance)."""
    H, W = _size(size, "camera_positions")
    Hs, Ws = _size(source_size, "camera_positions")
    if H < 2 or W < 2:
        raise ValueError("camera_positions: the grid needs at least 2 x 2 pixels, got %s" % ((H, W),))
    f = float(focal_px)
    if not np.isfinite(f) or f <= 0:
        raise ValueError("camera_positions: focal_px must be positive, got %r" % (focal_px,))
    cx, cy = (Ws / 2.0, Hs / 2.0) if principal is None else (float(principal[0]), float(principal[1]))
    s = float(light_size or 1.0)
    m = _homographies(homographies, None, "camera_positions")
    # x index = (X + s/2) (W - 1) / s, y index = (s/2 - Y) (H - 1) / s; continuous pixel = index + 0.5
    A = np.array([[(W - 1) / s, 0.0, (W - 1) / 2.0 + 0.5], [0.0, -(H - 1) / s, (H - 1) / 2.0 + 0.5], [0.0, 0.0, 1.0]])
    Kinv = np.array([[1.0 / f, 0.0, -cx / f], [0.0, 1.0 / f, -cy / f], [0.0, 0.0, 1.0]])
    out = np.empty((m.shape[0], 3))
    for l in range(m.shape[0]):
        G = Kinv @ m[l] @ A
        norm = 0.5 * (np.linalg.norm(G[:, 0]) + np.linalg.norm(G[:, 1]))
        if not np.isfinite(norm) or norm == 0.0 or G[2, 2] == 0.0:
            raise ValueError("camera_positions: homography %d is degenerate" % l)
        G = G / (norm if G[2, 2] > 0 else -norm)
        R = np.stack([G[:, 0], G[:, 1], np.cross(G[:, 0], G[:, 1])], axis=1)
        Uu, _, Vt = np.linalg.svd(R)
        R = Uu @ np.diag([1.0, 1.0, np.linalg.det(Uu @ Vt)]) @ Vt
        out[l] = -R.T @ G[:, 2]
    return torch.from_numpy(out)


_LIGHT_TYPES = {"directional": N.LIGHT_DIRECTIONAL, "point": N.LIGHT_POINT}


def _host_rows(v, what: str) -> np.ndarray:
    """A tensor on any device or a sequence -> float64 [rows,3] on the host (a device tensor is read back: one synchronisation)."""
    try:
        m = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if m.dtype.kind not in "fiu":
            raise TypeError
        m = m.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("photometric_stereo: %s must be numbers, got %r" % (what, type(v))) from None
    if m.ndim == 1 and m.shape[0] == 3:
        m = m[None]
    if m.ndim != 2 or m.shape[1] != 3 or m.shape[0] < 1:
        raise ValueError("photometric_stereo: %s must be [L,3]%s, got %s" % (what, " or [3]" if what == "light_intensity" else "", m.shape))
    return m


def photometric_stereo(targets: torch.Tensor, weights: Optional[torch.Tensor] = None, *, light, light_intensity, light_type: str = "point",
                       light_size: Optional[float] = None, targets_srgb: bool = True, iterations: int = 3, shadow_cos: float = 0.1,
                       min_condition: float = 1e-4, albedo_srgb: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """A rectified light stack -> (normal [3,H,W], albedo [3,H,W], confidence [1,H,W]), float32 on the targets' device: the maps to START a
    fit from, in one pass of csrc/photometric.hip (include/pbr_hip.h, pbr_photometric_stereo, is the definition).

    targets          [L,3,H,W] float32 on a ROCm device, 1 <= L <= 16 (`rectify`'s first result); made contiguous if it is not.
    weights          [L,1,H,W] (`rectify`'s second result), [1,1,H,W] (one plane for all shots) or None (all 1).  Another dtype (`bool` and
                     `uint8` masks included) or device is converted with `.to(float32)`, as the stack loss steps do.  A shot whose weight is
                     exactly 0 at a pixel is SKIPPED there, not multiplied by 0: a NaN target under a zero weight does no harm -- unlike the
                     loss steps, where 0 * NaN is NaN.
    light            [L,3]: point-light positions on the grid P = (xs, -ys, 0), xs, ys = linspace(-s/2, s/2, .), s = light_size or 1.0 --
                     the coordinates `cook_torrance(light_type="point")` uses -- or directions for light_type="directional".
    light_intensity  [3] / [1,3] for all shots, or [L,3]; every entry > 0.
                     Both may be tensors on any device or sequences; they are read to the HOST at the call and travel in the kernel's
                     arguments, so a device tensor costs a synchronisation -- acceptable for a step that runs once per fit.
    targets_srgb     the targets are sRGB-encoded (what `rectify` gives without to_linear, what return_srgb=True renders).
    iterations       1..4 solves: the first uses every shot, each later one masks the shots the solution before it puts in attached shadow
                     (w_l . n <= shadow_cos).  The clamp in N.L is what breaks linearity; on exactly Lambertian data with 17 % of the
                     observations shadowed one solve leaves 50.5 % of the pixels more than 0.01 degrees off, two 8.7 %, three none.
    shadow_cos       in [0, 1).
    min_condition    in (0, 1): a pixel whose normal matrix has det A / (tr A / 3)^3 below it (fewer than three independent lit shots) is
                     INVALID: normal exactly (0, 0, 1), confidence exactly 0, albedo from all its shots.  `confidence > 0` is the validity mask.
    albedo_srgb      sRGB-encode the albedo (what a material with albedo_is_srgb=True holds).

    The solve is Lambertian and view-independent: no camera enters, and a specular lobe biases it (a rough dielectric: half a degree in
    the median).  Not differentiable.  Every bad argument raises ValueError before any device work."""
    what = "photometric_stereo"
    if not isinstance(targets, torch.Tensor) or targets.dim() != 4 or targets.shape[1] != 3 or min(targets.shape) < 1:
        raise ValueError("%s: targets must be [L,3,H,W] (batched captures are not supported), got %s"
                         % (what, tuple(targets.shape) if isinstance(targets, torch.Tensor) else type(targets)))
    if targets.dtype != torch.float32:
        raise ValueError("%s: targets must be float32, got %s" % (what, targets.dtype))
    L, _, H, W = targets.shape
    if L > N.MAX_PHOTOMETRIC_SHOTS:
        raise ValueError("%s: at most %d shots, got %d" % (what, N.MAX_PHOTOMETRIC_SHOTS, L))
    shared = False
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or tuple(weights.shape) not in ((L, 1, H, W), (1, 1, H, W)):
            raise ValueError("%s: weights must be %s (one plane per shot) or %s (one plane for all shots), got %s"
                             % (what, (L, 1, H, W), (1, 1, H, W), tuple(weights.shape) if isinstance(weights, torch.Tensor) else type(weights)))
        shared = weights.shape[0] == 1 and L > 1
    if light_type not in _LIGHT_TYPES:
        raise ValueError("%s: light_type must be 'point' or 'directional', got %r" % (what, light_type))
    lights = _host_rows(light, "light")
    inten = _host_rows(light_intensity, "light_intensity")
    if lights.shape[0] != L:
        raise ValueError("%s: %d lights for %d shots" % (what, lights.shape[0], L))
    if inten.shape[0] not in (1, L):
        raise ValueError("%s: light_intensity must be [3], [1,3] or [%d,3], got %s" % (what, L, inten.shape))
    inten = np.ascontiguousarray(np.broadcast_to(inten, (L, 3)))
    if not np.isfinite(lights).all() or not np.isfinite(inten).all():
        raise ValueError("%s: a light or intensity entry is not finite" % what)
    if not (inten > 0).all() or not (inten.astype(np.float32) > 0).all():
        raise ValueError("%s: every light_intensity entry must be > 0" % what)
    size = float(light_size) if light_size else 0.0                                 # `light_size or 1.0`: None and 0 mean 1.0 (the library's rule)
    if not np.isfinite(size):
        raise ValueError("%s: light_size must be finite, got %r" % (what, light_size))
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= int(iterations) <= 4:
        raise ValueError("%s: iterations must be 1, 2, 3 or 4, got %r" % (what, iterations))
    tau, kappa = float(shadow_cos), float(min_condition)
    if not 0.0 <= tau < 1.0 or not np.float32(tau) < 1.0:
        raise ValueError("%s: shadow_cos must be in [0, 1), got %r" % (what, shadow_cos))
    if not 0.0 < kappa < 1.0 or not 0.0 < np.float32(kappa) < 1.0:
        raise ValueError("%s: min_condition must be in (0, 1), got %r" % (what, min_condition))
    if not targets.is_cuda:
        raise ValueError("%s: targets must be on a ROCm device, got %s (there is no CPU path)" % (what, targets.device))
    N.require_device()
    dev = targets.device
    t = targets.detach().contiguous()
    w = None if weights is None else weights.detach().to(dev, torch.float32).contiguous()
    normal = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    albedo = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    confidence = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    rows = (ctypes.c_float * (3 * L))(*lights.reshape(-1).tolist())
    ints = (ctypes.c_float * (3 * L))(*inten.reshape(-1).tolist())
    launch(dev, N.lib().pbr_photometric_stereo, t.data_ptr(), None if w is None else w.data_ptr(), 1 if shared else 0, L, H, W, rows, ints,
           _LIGHT_TYPES[light_type], size, 1 if targets_srgb else 0, int(iterations), tau, kappa, 1 if albedo_srgb else 0,
           normal.data_ptr(), albedo.data_ptr(), confidence.data_ptr())
    CALLS["photometric_stereo"] += 1
    return normal, albedo, confidence


def initial_material(targets: torch.Tensor, weights: Optional[torch.Tensor] = None, roughness: float = 0.5, **kwargs):
    """`photometric_stereo(targets, weights, **kwargs)` as the material a fit starts from: a BasecolorMetallicMaterial holding that normal,
    the albedo sRGB-encoded (albedo_is_srgb=True), a constant `roughness` plane and metallic 0 -- ready to have `requires_grad_` set on its
    maps and to go into MultiLightRenderingLoss.  `albedo_srgb` is not a keyword here: the material's albedo is always encoded."""
    from .materials import BasecolorMetallicMaterial
    if "albedo_srgb" in kwargs:
        raise ValueError("initial_material: the material's albedo is always sRGB-encoded; albedo_srgb is not an argument")
    rough = float(roughness)
    if not 0.0 <= rough <= 1.0:
        raise ValueError("initial_material: roughness must be in [0, 1], got %r" % (roughness,))
    normal, albedo, _ = photometric_stereo(targets, weights, albedo_srgb=True, **kwargs)
    H, W = albedo.shape[-2:]
    return BasecolorMetallicMaterial(albedo=albedo, albedo_is_srgb=True, normal=normal,
                                     roughness=torch.full((1, H, W), rough, dtype=torch.float32, device=albedo.device),
                                     metallic=torch.zeros((1, H, W), dtype=torch.float32, device=albedo.device))
