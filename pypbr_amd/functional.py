"""Tensor-level entry points of the MI355X Cook-Torrance path.

`cook_torrance` evaluates what the reference's CookTorranceBRDF.forward computes
(/root/reference/pypbr/models/cooktorrance.py:92-182) on raw planar maps with ONE
fused HIP kernel launch; the map-level classes in pypbr_amd.materials / .models
call into it.  torch is used for device memory and streams only: every number is
produced by libpbr_hip.so.

Build extensions over the reference:
  * a leading batch dimension: maps may be [B,C,H,W]; B > 1 equals a loop of calls;
  * several lights: `light` [L,3] with `light_intensity` [L,3]; each light's linear
    contribution is clamped to [0,1] (what one reference call does), contributions are
    summed, clamped, and encoded once;
  * fp16 map storage (fp32 arithmetic), optional fp16 output;
  * row bands: (y_offset, height_total) evaluate rows of a taller map (multi-GPU
    sharding of a single material);
  * `convert_to_diffuse_specular`: to_diffuse_specular_material (metallic.py:71-120)
    fused in front of the specular-workflow evaluation.

This module is the public namespace of the tensor-level API and holds the render path itself; the other kernel families live in private
sibling modules, one per file of csrc/, and their names are imported back below, so `functional.<name>` resolves as it always did:

  _dispatch     what all families share: dtype codes, tensor checks, LAUNCHES, `launch` / `ptr`       (the C ABI: _native.py)
  _upload       to_host, pack_maps, upload_packed, unpack_image, pack_image, download_samples           csrc/unpack.hip, pack_image.hip
  _map_ops      colour transfers, metallic <-> specular, resize, decode_normal                          csrc/map_ops.hip, resize.hip, resize_backward.hip
  _normal_ops   normal_from_height, transform_normals                                                   csrc/normal_ops.hip
  _height_ops   height_from_normal (around torch.fft.rfft2 / irfft2)                                     csrc/height_ops.hip
  _geometry     PlaneMap, fold_stages, check_crop, remap_planes                                         csrc/geometry.hip
  _packing      unpack_planes, pack_planes, the plane-op tables                                         csrc/packing.hip
  _rotate_ops   rotate_plan, rotate_indices, rotate_maps                                                csrc/rotation.hip
  capture       homography_from_corners, rectify, camera_positions (photographs -> targets and weights)  csrc/rectify.hip
  functional    descriptors, RenderPlan, cook_torrance, the autograd bridges, rendering_loss_mse,       csrc/ct_*.hip/.hpp, torch_ops.cpp
                light stacks (cook_torrance_stack, rendering_loss_mse_stack)

The one-pass loss steps (_MseStepFn and the six light-stack classes, which take optional per-pixel weights) are autograd classes over one frame, said
once in front of _MseStepFn: two predicates for the callers (_shared_by_batch, _plain_kwargs), one table of step kinds (_KINDS), one launch
(_step_plan, _launch_loss_step), one ctx idiom (_keep_step, _kept_step) and the one scaling launch (_scale_step_gradients).  The six stack
classes are built by one factory (_stack_step_class) from (name, kind, takes_params, fit, doc); one route (_route, by the family's view type)
and one helper (_one_pass_loss) choose and apply them.

Imports run one way: _native / _caches -> _dispatch -> _upload -> the family modules -> functional.
"""
# Settings are assigned on the module that READS them.  USE_TORCH_OPS and DEVICE_PARAMETERS are read here.  PINNED_RESULT_CAP,
# PLANE_SKEW_BYTES, STAGE_MEMCPY_LIMIT and UPLOAD_STAGE_CAP are read by _upload and are deliberately NOT re-exported: an assignment to
# `functional.PLANE_SKEW_BYTES` would bind a name nobody reads, so reading it here raises AttributeError instead.  Likewise a
# monkeypatch of a helper that moved code calls inside its own module (_resize_raw, _stage_copy, _plane_ops_call ...) goes on that module.
import collections
import ctypes
import threading
from typing import Optional, Sequence, Tuple, Union

import torch

from . import _native as N
from ._caches import CACHING, KeptPlan, ValueMemo, VersionMemo, host_values, set_caching, version_of  # noqa: F401  (the settings are re-exported)
from ._dispatch import LAUNCHES, _DTYPES, _device_tensor, _grad_like, _needs_grad, _rows_dense, _stream_ptr, launch, ptr  # noqa: F401
from ._upload import (  # noqa: F401
    ENCODED_DTYPES, _PINNED_OUT, _UPLOAD_STAGE, _aligned_arena, _dense_samples, _pack_material_major, _page_locked_range, _stage_copy, _staged,
    _upload_stage, download_samples, is_encoded, pack_image, pack_maps, release_upload_stage, to_host, unpack_image, upload_packed)
from ._map_ops import (  # noqa: F401
    _ColourFn, _DecodeNormalFn, _MetallicToSpecularFn, _ResizeFn, _SpecularToMetallicFn, _colour_raw, _decode_normal_raw, _ds2bm_raw, _m2ds_raw,
    _resize_raw, decode_normal, diffuse_specular_to_basecolor_metallic, linear_to_srgb, metallic_to_diffuse_specular, resize, srgb_to_linear)
from ._normal_ops import (  # noqa: F401
    _NormalFromHeightFn, _TransformNormalsFn, _directx, _matrix, _nfh_raw, _transform_raw, normal_from_height, transform_normals)
from ._height_ops import _HeightFromNormalFn, _hfn_raw, _poisson_solve, height_from_normal  # noqa: F401
from ._geometry import PlaneMap, _RemapFn, _axis_map, _remap_raw, check_crop, fold_stages, remap_planes  # noqa: F401
from ._packing import (  # noqa: F401
    _PackFn, _UnpackFn, _affine_plan, _on_device, _pack, _pack_raw, _plane_ops_call, _plane_ptr, _planes_of, _run_plane_ops, _unpack_layout,
    _unpack_raw, pack_planes, unpack_planes)
from ._rotate_ops import (  # noqa: F401
    PADDING_MODES, _ROTATE_PLANS, RotatePlan, _RotateFn, _make_rotate_plan, _rotate_geom, _rotate_raw, rotate_indices, rotate_maps, rotate_plan)
from .capture import camera_positions, homography_from_corners, rectify  # noqa: F401

TensorLike = Union[torch.Tensor, Sequence[float]]

_LIGHT_TYPES = {"directional": N.LIGHT_DIRECTIONAL, "point": N.LIGHT_POINT}
_VIEW_TYPES = ("directional", "point")


def _view_type(kw) -> str:
    """`view_type` of a call's keyword arguments.  "directional" (the default, upstream's behaviour): `view_dir` is one direction for the whole
    image, an orthographic camera.  "point": `view_dir` is a camera POSITION in the point light's coordinates and every pixel looks towards it
    (csrc/ct_camera.hip) -- whole untiled maps or row bands of them, a float32 result, no fused blend.  Pure host logic: raises before any
    device is asked for."""
    vt = str(kw.get("view_type", "directional")).lower()
    if vt not in _VIEW_TYPES:
        raise ValueError(f"Unsupported view_type: {vt}. Must be 'directional' or 'point'.")
    if vt == "point":
        if tile_counts(kw.get("tile", 1)) != (1, 1) or kw.get("rows") is not None:
            raise NotImplementedError("view_type='point' renders untiled maps (tile=1): materialise the repeats first")
        if kw.get("blend") is not None:
            raise NotImplementedError("view_type='point' takes no fused blend: blend the materials first")
        out = kw.get("out")
        if kw.get("out_dtype") not in (None, torch.float32) or (isinstance(out, torch.Tensor) and out.dtype != torch.float32):
            raise NotImplementedError("view_type='point' gives a float32 result (fp16 maps are fine)")
    return vt


# The caches' settings live in _caches (what they recognise as "did not change", and why all three are off by default, is said there).
_HOST_COPIES = VersionMemo()          # host copies of device-resident parameter tensors


def _host_vec3(v: TensorLike, rows: Optional[int] = None):
    """Host values of a light / view parameter for the kernel-argument segment.  Tensors that live on a ROCm device do NOT come here any more
    (DEVICE_PARAMETERS: the kernels read them from device memory, _device_parameter_tensors); with that switched off a device tensor costs one
    small blocking D2H copy per call, as the reference's `.to(device)` / scalar reads do, and with
    `set_caching(parameters=True)` the host values are remembered per tensor object and version counter, so a caller
    that keeps its light / view tensors on the GPU and passes the same unchanged tensors call after call (the
    reference's override_device usage) synchronises on the first call only.  Tensors that require grad are read
    detached; their gradient comes from the backward kernel (see _CookTorranceFn)."""
    if not isinstance(v, torch.Tensor):
        t = torch.as_tensor(v, dtype=torch.float32)
    elif v.is_cuda:
        ver = version_of(v) if CACHING["parameters"] else None
        t = _HOST_COPIES.get(v, ver) if ver is not None else None
        if t is None:
            t = v.detach().to("cpu", torch.float32)
            if ver is not None:
                _HOST_COPIES.put(v, ver, t)
    else:
        t = v.detach().to(torch.float32)
    if rows is None:
        if t.numel() != 3:
            raise ValueError("expected a vector of 3 components, got shape %s" % (tuple(t.shape),))
        return [float(x) for x in t.reshape(3).tolist()]
    t = t.reshape(-1, 3)
    return [[float(x) for x in r] for r in t.tolist()]


DEVICE_PARAMETERS = True     # view / light / intensity tensors that live on the device are read there (pbr_render_desc.device_params), not copied to the host


_WARNED_PARAMETER_COPY = []


def _warn_parameter_copy(t, device):
    """A device-resident parameter that is not float32 / contiguous / on the maps' device is read through a COPY made now: later
    edits of the tensor (an optimiser step, a graph replay) are not seen by a plan built from it.  Said once."""
    if not _WARNED_PARAMETER_COPY:
        _WARNED_PARAMETER_COPY.append(True)
        import warnings
        warnings.warn("pypbr_amd: a view / light / intensity tensor (%s, %s on %s) is not a contiguous float32 tensor on the maps' device (%s); "
                      "the kernels read a copy made at planning time, so a RenderPlan or captured graph will not see later updates of it"
                      % (tuple(t.shape), t.dtype, t.device, device), stacklevel=3)


def _device_parameter_tensors(view_dir, light, light_intensity, device):
    """When one of view_dir / light / light_intensity is a tensor on a ROCm device: (view [3] | None, lights [L,3] | None, intensities [1|L,3] | None)
    -- the device-resident ones as contiguous float32 tensors on `device`, None for those the caller holds on the host (they travel in the
    descriptor as always).  The kernels then read the device ones from device memory: no blocking read-back, no copy in either direction, and a
    captured graph sees the tensors' CURRENT values at every replay (a light being fitted by an optimiser).  Else None."""
    if not DEVICE_PARAMETERS or not any(isinstance(t, torch.Tensor) and t.is_cuda for t in (view_dir, light, light_intensity)):
        return None
    on_device = lambda t: isinstance(t, torch.Tensor) and t.is_cuda

    def conv(t, rows):
        if not on_device(t):
            return None
        c = t.detach().to(device, torch.float32).reshape(rows).contiguous()
        if c.data_ptr() != t.data_ptr():
            _warn_parameter_copy(t, device)
        return c
    v, lt, it = conv(view_dir, (-1,)), conv(light, (-1, 3)), conv(light_intensity, (-1, 3))
    if v is not None and v.numel() != 3:
        raise ValueError("expected a vector of 3 components, got shape %s" % (tuple(v.shape),))
    return v, lt, it


def _as_batched(t: Optional[torch.Tensor], channels: Tuple[int, ...], name: str):
    if t is None:
        return None
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] not in channels:
        raise ValueError("%s must be [%s,H,W] or [B,%s,H,W], got %s" % (name, channels, channels, tuple(t.shape)))
    if t.stride(-1) != 1 or t.stride(-2) != t.shape[-1]:   # rows must be contiguous; planes/batches may be strided
        t = t.contiguous()
    return t


def _pbr_map(t: Optional[torch.Tensor]) -> N.PbrMap:
    if t is None:
        return N.PbrMap(None, 0, 0)
    return N.PbrMap(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else 0, t.stride(1))


def tile_counts(tile) -> Tuple[int, int]:
    """MaterialBase.tile(num_tiles) repeats both axes num_tiles times (base.py:524-537); (ny, nx) is accepted too."""
    ny, nx = (tile, tile) if isinstance(tile, int) else (int(tile[0]), int(tile[1]))
    if ny < 1 or nx < 1:
        raise ValueError("tile counts must be >= 1, got %s" % (tile,))
    return ny, nx


def build_descriptor(albedo, normal, roughness, metallic, specular, out, *, view_dir, light, light_intensity,
                     light_type, light_size, albedo_is_srgb, specular_is_srgb, return_srgb,
                     convert_to_diffuse_specular, y_offset, height_total, schedule=0, tile=(1, 1)) -> N.RenderDesc:
    """Fills the C-ABI descriptor (include/pbr_hip.h: pbr_render_desc) from [B,C,H,W] tensors.
    Pure host logic: no device access, so it is testable without a GPU.  `tile=(ny, nx)` != (1, 1): the maps
    repeat over a (ny*H, nx*W) output (wrap-around addressing); `out` [B,3,rows,nx*W] then holds the rows
    [y_offset, y_offset + rows) of it."""
    lt = str(light_type).lower()
    if lt not in _LIGHT_TYPES:   # cooktorrance.py:62-65
        raise ValueError(f"Unsupported light_type: {lt}. Must be 'directional' or 'point'.")
    if metallic is not None:
        workflow = N.WORKFLOW_CONVERTED if convert_to_diffuse_specular else N.WORKFLOW_METALLIC
    elif specular is not None:
        if convert_to_diffuse_specular:
            raise ValueError("convert_to_diffuse_specular needs a metallic map")
        workflow = N.WORKFLOW_SPECULAR
    else:                         # cooktorrance.py:115-118
        raise ValueError("Material must have either 'metallic' or 'specular' property.")

    B, _, H, W = albedo.shape
    for name, t in (("normal", normal), ("roughness", roughness), ("metallic", metallic), ("specular", specular)):
        if t is None:
            continue
        if t.shape[-2:] != (H, W) or t.shape[0] not in (1, B):
            raise ValueError("%s %s does not match albedo %s" % (name, tuple(t.shape), tuple(albedo.shape)))
        if t.dtype != albedo.dtype or t.device != albedo.device:
            raise TypeError("all maps must share dtype and device (%s is %s on %s)" % (name, t.dtype, t.device))
    if albedo.dtype not in _DTYPES or out.dtype not in _DTYPES:
        raise TypeError("maps must be float32 or float16, got %s" % albedo.dtype)

    dev_params = _device_parameter_tensors(view_dir, light, light_intensity, albedo.device)
    # parameters that live on the device stay there (pbr_prepare_device_params, plan_cook_torrance); the others travel in the descriptor
    dv, dl, di = dev_params if dev_params is not None else (None, None, None)
    lights = [[0.0, 0.0, 0.0]] * dl.shape[0] if dl is not None else _host_vec3(light, rows=-1)
    intens = [[0.0, 0.0, 0.0]] * di.shape[0] if di is not None else _host_vec3(light_intensity, rows=-1)
    if dv is not None:
        view_dir = [0.0, 0.0, 1.0]
    if len(intens) == 1 and len(lights) > 1:
        intens = intens * len(lights)
    if len(lights) != len(intens):
        raise ValueError("light [%d,3] and light_intensity [%d,3] disagree" % (len(lights), len(intens)))
    if not 1 <= len(lights) <= N.MAX_LIGHTS:
        raise ValueError("between 1 and %d lights are supported, got %d" % (N.MAX_LIGHTS, len(lights)))

    d = N.RenderDesc()
    d.abi_version = N.ABI_VERSION
    ny, nx = tile_counts(tile)
    if (ny, nx) == (1, 1):
        d.batch, d.height, d.width = B, H, W
        d.height_total = H if height_total is None else int(height_total)
    else:
        if height_total not in (None, ny * H):
            raise ValueError("with tile=%s the full map has %d rows, not height_total=%s" % ((ny, nx), ny * H, height_total))
        d.batch, d.height, d.width = B, out.shape[-2], nx * W
        d.height_total, d.map_height, d.map_width = ny * H, H, W
        if tuple(out.shape[-2:]) != (d.height, d.width) or int(y_offset) + d.height > d.height_total:
            raise ValueError("out %s is not a band of the tiled %dx%d map" % (tuple(out.shape), ny * H, nx * W))
    d.y_offset = int(y_offset)
    d.map_dtype, d.out_dtype = _DTYPES[albedo.dtype], _DTYPES[out.dtype]
    d.workflow, d.light_type, d.n_lights = workflow, _LIGHT_TYPES[lt], len(lights)
    d.albedo_is_srgb = int(bool(albedo_is_srgb))
    d.specular_is_srgb = int(bool(specular_is_srgb))
    d.return_srgb = int(bool(return_srgb))
    d.albedo, d.normal, d.roughness = _pbr_map(albedo), _pbr_map(normal), _pbr_map(roughness)
    d.metallic, d.specular = _pbr_map(metallic), _pbr_map(specular)
    d.out = out.data_ptr()
    if out.dim() == 4 and not out.is_contiguous():      # rows contiguous (checked by the caller); planes / materials strided
        d.out_batch_stride = out.stride(0) if out.shape[0] > 1 else 0
        d.out_channel_stride = out.stride(1)
    v = _host_vec3(view_dir)
    for c in range(3):
        d.view_dir[c] = v[c]
    d.light_size = float(light_size) if light_size else 0.0   # falsy -> 1.0 inside (cooktorrance.py:130)
    d.schedule = int(schedule)
    for i, (l, it) in enumerate(zip(lights, intens)):
        for c in range(3):
            d.lights[i][c] = l[c]
            d.intensities[i][c] = it[c]
    d._device_parameters = dev_params          # (view [3], lights [L,3], intensities [1|L,3]) on the maps' device, or None
    return d


def refill_parameters(d, view_dir, light, light_intensity):
    """Host values of view / light / intensity into an existing descriptor (same number of lights): what build_descriptor writes."""
    v = _host_vec3(view_dir)
    lights, intens = _host_vec3(light, rows=-1), _host_vec3(light_intensity, rows=-1)
    if len(intens) == 1 and len(lights) > 1:
        intens = intens * len(lights)
    if len(lights) != len(intens) or len(lights) != d.n_lights:
        raise ValueError("light [%d,3] and light_intensity [%d,3] disagree with the descriptor's %d lights" % (len(lights), len(intens), d.n_lights))
    for c in range(3):
        d.view_dir[c] = v[c]
    for i, (l, it) in enumerate(zip(lights, intens)):
        for c in range(3):
            d.lights[i][c] = l[c]
            d.intensities[i][c] = it[c]


class RenderPlan:
    """A filled descriptor plus the tensors it points into: `launch()` is one C-ABI call
    (ctypes + hipLaunchKernel, a few microseconds), for callers that evaluate the same
    maps repeatedly (bench.py, a rendering-loss loop) and must not pay the Python-side
    descriptor construction per step."""

    def __init__(self, desc, out, keep_alive, squeeze, view_type="directional"):
        self.desc, self.out, self._keep, self._squeeze = desc, out, keep_alive, squeeze
        self.device = out.device
        self._second_given = keep_alive[3] is not None or keep_alive[4] is not None    # a metallic or specular map (a kept plan empties _keep)
        self.view_type = view_type                          # "point": desc.view_dir is a camera position, launched through pbr_cook_torrance_camera
        self._fn = N.lib().pbr_cook_torrance_camera if view_type == "point" else N.lib().pbr_cook_torrance
        self._ref = ctypes.byref(desc)
        self._param_tensors = (None, None, None)            # device-resident view / lights / intensities (prepare_device_parameters)
        self._param_block, self._param_stream = None, None

    @property
    def result(self) -> torch.Tensor:
        return self.out[0] if self._squeeze else self.out

    @property
    def kernel_name(self) -> str:
        return N.lib().pbr_kernel_name(self._ref).decode()

    @property
    def bytes_per_pixel(self) -> int:
        return N.lib().pbr_bytes_per_pixel(self._ref)

    def set_tuning(self, **knobs):
        """Per-call schedule knobs of THIS plan (pbr_render_desc.tuning; names of _native.TUNE_NAMES, e.g. lds_bytes=0, block_log2=8):
        they travel with the descriptor, touch no process-wide state and change speed only, never results.  No arguments: back to the rules."""
        if knobs:
            self._tuning = N.Tuning.of(**knobs)
            self.desc.tuning = ctypes.pointer(self._tuning)
        else:
            self._tuning = None
            self.desc.tuning = None
        return self

    def autotune(self, stream: Optional[int] = None) -> int:
        """pbr_cook_torrance_autotune on this plan's buffers: blocks, rewrites `out`, stores and returns the
        fastest schedule.  Not inside a stream capture."""
        best = ctypes.c_int32(0)
        with torch.cuda.device(self.device):
            N.check(N.lib().pbr_cook_torrance_autotune(self._ref, _stream_ptr(self.device) if stream is None else stream,
                                                       ctypes.byref(best)))
        self.desc.schedule = best.value
        return best.value

    def prepare_device_parameters(self, tensors=None, stream: Optional[int] = None):
        """pbr_prepare_device_params: folds view / light / intensity tensors that live on the device into the block the kernels read
        (enqueued on the stream; no host access to their values).  Called by plan_cook_torrance; call it again -- or capture it in a graph
        in front of `launch()` -- after the tensors changed (`tensors` = (view [3] | None, lights [L,3] | None, intensities [1|L,3] | None) to switch to others; None = the
        descriptor's host values)."""
        if tensors is not None:
            self._param_tensors = tuple(tensors)
        v, lt, it = self._param_tensors
        lib = N.lib()
        if self._param_block is None:
            self._param_block = torch.empty((lib.pbr_device_params_bytes() + 3) // 4, dtype=torch.float32, device=self.device)
        if (lt is not None and lt.shape[0] != self.desc.n_lights) or (it is not None and it.shape[0] not in (1, self.desc.n_lights)):
            raise ValueError("light / light_intensity rows disagree with the descriptor's %d lights" % self.desc.n_lights)
        st = _stream_ptr(self.device) if stream is None else stream
        with torch.cuda.device(self.device):
            N.check(lib.pbr_prepare_device_params(self._ref, ptr(v), ptr(lt), ptr(it), 1 if it is None else it.shape[0], self._param_block.data_ptr(), st))
        self.desc.device_params = self._param_block.data_ptr()
        self._param_stream = st                             # launches on another stream fold the parameters again there (launch)

    def refill(self, view_dir, light, light_intensity) -> bool:
        """refill_parameters on this plan's descriptor; False, and nothing written, when the values do not fit it (another number of lights)."""
        try:
            refill_parameters(self.desc, view_dir, light, light_intensity)
        except ValueError:
            return False
        return True

    def attach_blend(self, blend_desc, workspace, keep_alive):
        """Turns the plan into blend + evaluate (pbr_cook_torrance_blend): material 2 and the mask."""
        self._blend, self._blend_ref, self._workspace = blend_desc, ctypes.byref(blend_desc), workspace
        self._keep = self._keep + tuple(keep_alive)

    def blend_normal_sign(self, stream: Optional[int] = None) -> torch.Tensor:
        """pbr_blend_normal_sign over the rows this plan holds: an int32 [B] tensor, 1 where the blended normal of
        material b has a negative component there.  For row bands: combine the bands' flags (max) and hand them to the
        plans as `blend_flags`."""
        if getattr(self, "_blend", None) is None:
            raise ValueError("not a blend plan")
        flags = torch.zeros(self.desc.batch, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().pbr_blend_normal_sign(self._ref, self._blend_ref, flags.data_ptr(),
                                                  _stream_ptr(self.device) if stream is None else stream))
        return flags

    def use_blend_flags(self, flags: torch.Tensor):
        """Whole-map flags worked out by the caller (see `blend_normal_sign`)."""
        self._blend.sign_mode = N.BLEND_SIGN_GIVEN
        self._workspace = flags.to(self.device, torch.int32).contiguous()

    def launch(self, stream: Optional[int] = None) -> torch.Tensor:
        """Enqueue on `stream` (raw hipStream_t) or torch's current stream of the maps' device."""
        if self.out.numel() == 0 and self._second_given:
            return self.result         # zero-sized maps: the reference's whole-map ops return an empty (3, H, W) image; nothing to enqueue
        st = _stream_ptr(self.device) if stream is None else stream
        if self._param_stream is not None and st != self._param_stream:
            # the parameter block was written by a kernel on ANOTHER stream: nothing orders this launch behind it.  Folding the
            # parameters again on the launch stream (one wave) does, and picks up the tensors' current values.
            self.prepare_device_parameters(stream=st)
        if getattr(self, "_blend", None) is not None:
            rc = N.lib().pbr_cook_torrance_blend(self._ref, self._blend_ref, self._workspace.data_ptr(), st)
        else:
            rc = self._fn(self._ref, st)
        if rc != N.OK:
            N.check(rc)
        return self.result


def plan_cook_torrance(albedo: torch.Tensor, normal: Optional[torch.Tensor], roughness: torch.Tensor,
                       metallic: Optional[torch.Tensor] = None, specular: Optional[torch.Tensor] = None, *,
                       view_dir: TensorLike, light: TensorLike, light_intensity: TensorLike,
                       light_type: str = "point", light_size: Optional[float] = None,
                       albedo_is_srgb: bool = True, specular_is_srgb: bool = True, return_srgb: bool = True,
                       convert_to_diffuse_specular: bool = False, y_offset: int = 0,
                       height_total: Optional[int] = None, out_dtype: Optional[torch.dtype] = None,
                       out: Optional[torch.Tensor] = None, schedule: int = N.SCHEDULE_AUTO,
                       autotune: bool = False, tile=1, rows: Optional[int] = None,
                       blend: Optional[Sequence[Optional[torch.Tensor]]] = None,
                       blend_flags: Optional[torch.Tensor] = None, tuning: Optional[dict] = None,
                       view_type: str = "directional") -> RenderPlan:
    """Validates the maps, allocates the output and fills the C-ABI descriptor; see `cook_torrance`.
    `schedule`: workgroup order (N.SCHEDULE_AUTO | N.SCHEDULE_LINEAR | N.schedule_xcd(c)), results do not depend
    on it; `autotune=True` measures the candidates on these very buffers once (blocking, a few launches) and
    keeps the fastest -- for plans that are launched many times.
    `tile=n | (ny, nx)`: evaluate `material.tile(n)` (base.py:524-537) without materialising the repeated maps --
    the kernel wraps its texel addresses, so each texel leaves HBM once instead of ny*nx times; the result is the
    (ny*H, nx*W) image (or its rows [y_offset, y_offset + rows)).
    `blend=(albedo2, normal2, roughness2, metallic2, specular2, mask)`: blend_with_mask (blending/functional.py:64-145:
    mask * map1 + (1 - mask) * map2, normals normalised / blended / normalised, the blended normal re-decoded as on
    assignment) fused in front of the evaluation -- both materials are read once, the blended maps are never written.
    fp32 maps, both materials complete; `mask` [1,H,W] or [B,1,H,W].  Whether a blended normal map counts as already
    signed is decided over the WHOLE map (base.py:212); the launch works that out itself unless the maps are a row band
    of a taller untiled map -- then pass `blend_flags` (int32 [B] on the device: `RenderPlan.blend_normal_sign()` of
    every band, combined with max; distributed.cook_torrance_sharded does this).
    `tuning={"lds_bytes": 0, ...}`: per-call schedule knobs of this plan (RenderPlan.set_tuning); speed only, never results.
    `view_type="point"`: `view_dir` is the camera's position (`_view_type`); the plan launches pbr_cook_torrance_camera, and a position that
    lives on the device is read there at every launch, like any device-resident parameter."""
    view_type = _view_type(dict(view_type=view_type, tile=tile, rows=rows, blend=blend, out_dtype=out_dtype, out=out))
    if not isinstance(albedo, torch.Tensor) or not albedo.is_cuda:
        raise RuntimeError("pypbr_amd.functional.cook_torrance needs maps on a ROCm device "
                           "(use material.to('cuda')); there is no CPU path")
    squeeze = albedo.dim() == 3
    a = _as_batched(albedo, (3,), "albedo")
    n = _as_batched(normal, (3,), "normal")
    r = _as_batched(roughness, (1,), "roughness")
    m = _as_batched(metallic, (1,), "metallic")
    s = _as_batched(specular, (3,), "specular")
    B, _, H, W = a.shape
    ny, nx = tile_counts(tile)
    if (ny, nx) != (1, 1):
        H, W = (ny * H - int(y_offset)) if rows is None else int(rows), nx * W
    elif rows is not None:
        raise ValueError("`rows` selects a band of a tiled map; without `tile` pass the band's own maps")
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=out_dtype or torch.float32, device=a.device)
    elif (tuple(out.shape[-3:]) != (3, H, W) or out.device != a.device or out.stride(-1) != 1 or out.stride(-2) != W
          or (out.dim() == 4 and out.shape[0] != B) or out.dim() not in (3, 4)):
        raise ValueError("out must be a [B,3,H,W] tensor with contiguous rows on the maps' device")
    if out.dim() == 3:
        out = out.unsqueeze(0)
    desc = build_descriptor(a, n, r, m, s, out, view_dir=view_dir, light=light, light_intensity=light_intensity,
                            light_type=light_type, light_size=light_size, albedo_is_srgb=albedo_is_srgb,
                            specular_is_srgb=specular_is_srgb, return_srgb=return_srgb,
                            convert_to_diffuse_specular=convert_to_diffuse_specular, y_offset=y_offset,
                            height_total=height_total, schedule=schedule, tile=(ny, nx))
    plan = RenderPlan(desc, out, (a, n, r, m, s), squeeze and out.dim() == 4, view_type)
    if tuning:
        plan.set_tuning(**tuning)
    if desc._device_parameters is not None:
        plan.prepare_device_parameters(desc._device_parameters)
    if blend is not None:
        if len(blend) != 6:
            raise ValueError("blend = (albedo2, normal2, roughness2, metallic2, specular2, mask)")
        if a.dtype != torch.float32 or out.dtype != torch.float32:
            raise TypeError("the fused blend supports float32 maps and output")
        if n is None:
            raise ValueError("the fused blend needs a normal map in both materials")
        a2, n2, r2 = (_as_batched(blend[0], (3,), "albedo2"), _as_batched(blend[1], (3,), "normal2"),
                      _as_batched(blend[2], (1,), "roughness2"))
        m2, s2 = _as_batched(blend[3], (1,), "metallic2"), _as_batched(blend[4], (3,), "specular2")
        k = _as_batched(blend[5] if blend[5].dim() != 2 else blend[5].unsqueeze(0), (1,), "mask")
        second = m2 if m is not None else s2
        if a2 is None or n2 is None or r2 is None or second is None or k is None:
            raise ValueError("the fused blend needs albedo, normal, roughness and %s of material 2 and a mask"
                             % ("metallic" if m is not None else "specular"))
        for name, t, like in (("albedo2", a2, a), ("normal2", n2, n), ("roughness2", r2, r), ("metallic2|specular2", second, m if m is not None else s),
                              ("mask", k, r)):
            if t.shape[-2:] != like.shape[-2:] or t.shape[0] not in (1, B) or t.dtype != torch.float32 or t.device != a.device:
                raise ValueError("%s %s (%s on %s) does not match material 1" % (name, tuple(t.shape), t.dtype, t.device))
        bd = N.BlendDesc()
        bd.albedo, bd.normal, bd.roughness = _pbr_map(a2), _pbr_map(n2), _pbr_map(r2)
        bd.metallic = _pbr_map(m2 if m is not None else None)
        bd.specular = _pbr_map(s2 if m is None else None)
        bd.mask = _pbr_map(k)
        if blend_flags is not None:
            if blend_flags.dtype != torch.int32 or blend_flags.numel() != B or blend_flags.device != a.device:
                raise ValueError("blend_flags must be an int32 tensor of %d flags on the maps' device" % B)
            bd.sign_mode = N.BLEND_SIGN_GIVEN
            flags = blend_flags.contiguous()
        else:
            flags = torch.empty(B, dtype=torch.int32, device=a.device)
        plan.attach_blend(bd, flags, (a2, n2, r2, second, k))
    elif autotune and view_type != "point":                 # (the schedules pbr_cook_torrance_autotune times are the orthographic kernels')
        plan.autotune()
    return plan


def cook_torrance(albedo: torch.Tensor, normal: Optional[torch.Tensor], roughness: torch.Tensor,
                  metallic: Optional[torch.Tensor] = None, specular: Optional[torch.Tensor] = None,
                  **kwargs) -> torch.Tensor:
    """Fused Cook-Torrance evaluation on device-resident planar maps.

    albedo/normal/specular: [3,H,W] or [B,3,H,W]; roughness/metallic: [1,H,W] or
    [B,1,H,W]; all on one ROCm device, float32 or float16.  Keyword arguments:
    view_dir, light, light_intensity (required), light_type="point", light_size=None,
    albedo_is_srgb=True, specular_is_srgb=True, return_srgb=True,
    convert_to_diffuse_specular=False, y_offset=0, height_total=None, out_dtype=None, out=None,
    schedule=0, autotune=False, tile=1, rows=None, blend=None, blend_flags=None, view_type="directional" (see `plan_cook_torrance`;
    with view_type="point" `view_dir` is a camera position and its gradient the position's).
    Returns [3,H,W] or [B,3,H,W] (float32 unless `out_dtype`), on the same device,
    enqueued on the current stream without synchronising.  Differentiable with respect to the maps and to
    view_dir / light / light_intensity when those are tensors that require grad (backward kernels); the plain
    evaluation goes through `torch.ops.pbr_hip.cook_torrance` when that extension is built, through the ctypes
    binding of the same C ABI otherwise (and for out= / schedule= / autotune= / blend=).
    """
    _view_type(kwargs)
    if kwargs.get("blend") is not None and torch.is_grad_enabled() and any(
            isinstance(t, torch.Tensor) and t.requires_grad
            for t in (albedo, normal, roughness, metallic, specular) + tuple(kwargs["blend"]) + tuple(kwargs.get(k) for k in _PARAM_KEYS)):
        if _fused_blend_backward_can_take(albedo, kwargs):
            kw = {k: v for k, v in kwargs.items() if k != "blend"}
            try:
                return _FusedBlendFn.apply(kw, albedo, normal, roughness, metallic, specular, *kwargs["blend"])
            except _StepNotServed:
                pass
        return _blend_then_render_with_grad(albedo, normal, roughness, metallic, specular, **kwargs)
    if USE_TORCH_OPS and _torch_op_can_take(albedo, kwargs):
        return _cook_torrance_via_torch_op(albedo, normal, roughness, metallic, specular, **kwargs)
    maps = (albedo, normal, roughness, metallic, specular)
    params = tuple(kwargs.get(k) for k in _PARAM_KEYS)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in maps + params):
        kw = {k: v for k, v in kwargs.items() if k not in _PARAM_KEYS}
        return _CookTorranceFn.apply(albedo, normal, roughness, metallic, specular, *params, kw)
    plan = plan_cook_torrance(albedo, normal, roughness, metallic, specular, **kwargs)
    with torch.cuda.device(plan.device):
        return plan.launch()


def _fused_blend_backward_can_take(albedo, kw) -> bool:
    """pbr_cook_torrance_blend_backward covers gradients of the maps of both materials and of the mask: fp32, untiled, a fresh
    result.  Gradients of view / light parameters through a blend take the unfused differentiable pieces."""
    if kw.get("out") is not None or kw.get("out_dtype") not in (None, torch.float32):
        return False
    if any(isinstance(kw.get(k), torch.Tensor) and kw[k].requires_grad for k in _PARAM_KEYS):
        return False
    tensors = [albedo] + [t for t in kw["blend"] if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return False
    if kw.get("tile", 1) not in (1, (1, 1)):
        # tiled maps (round 6, ABI 8): every map with its own planes here (a shared map would own a sum over the batch of MAP-sized planes);
        # the library answers the rest when the plan exists (pbr_blend_backward_serves: one light, map rows of whole 4-texel groups, a whole
        # output or a band that holds a period of the map's rows) -- _FusedBlendFn.forward raises _StepNotServed and the unfused pieces run
        B = albedo.shape[0] if albedo.dim() == 4 else 1
        if any(_shared_by_batch(t, B) for t in tensors):
            return False
    return True


class _FusedBlendFn(torch.autograd.Function):
    """blend_with_mask -> re-assignment of the blended normal -> CookTorranceBRDF.forward as ONE kernel forward
    (pbr_cook_torrance_blend) and ONE kernel backward (pbr_cook_torrance_blend_backward): the gradients of both materials' maps
    and of the mask, what the reference's autograd derives through examples/example_blend.py:14-32 inside a rendering loss."""

    @staticmethod
    def forward(ctx, kwargs, *tensors):
        maps, blend = tensors[:5], tensors[5:11]
        det = lambda t: None if t is None else t.detach()
        plan = plan_cook_torrance(*[det(t) for t in maps], blend=tuple(det(t) for t in blend), **kwargs)
        if plan.desc.map_height and not N.lib().pbr_blend_backward_serves(ctypes.byref(plan.desc)):
            raise _StepNotServed()                                # tiled, and not a launch of the fused tiled backward: the caller's unfused pieces
        ctx.plan = plan
        ctx.shapes = [None if t is None else tuple(t.shape) for t in tensors]
        ctx.save_for_backward(*[t for t in tensors if t is not None])   # for autograd's in-place-modification check
        with torch.cuda.device(plan.device):
            result = plan.launch()
        plan.out = None
        return result

    @staticmethod
    def backward(ctx, grad_out):
        ctx.saved_tensors
        plan = ctx.plan
        d = plan.desc
        B, H, W = d.batch, d.height, d.width
        g = grad_out.reshape(B, 3, H, W).to(torch.float32).contiguous()
        if d.map_height and (d.map_height != d.height_total or d.map_width != d.width):
            H, W = d.map_height, d.map_width                      # tiled maps: MAP-sized gradients, every texel's sum over its repeats
        dev = g.device
        channels = (3, 3, 1, 1, 3)
        need = ctx.needs_input_grad[1:]                       # [0] is the kwargs dict

        def bufs(offset):
            out = []
            for i in range(5):
                want = need[offset + i] and ctx.shapes[offset + i] is not None
                out.append(torch.empty((B, channels[i], H, W), dtype=torch.float32, device=dev) if want else None)
            return out
        b1, b2 = bufs(0), bufs(5)
        gmask = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if need[10] else None
        G1, G2 = N.MapGrads(*[ptr(b) for b in b1]), N.MapGrads(*[ptr(b) for b in b2])
        bd = N.BlendDesc.from_buffer_copy(plan._blend)        # the flags the forward launch left in the workspace are the whole map's
        bd.sign_mode = N.BLEND_SIGN_GIVEN
        launch(dev, N.lib().pbr_cook_torrance_blend_backward, ctypes.byref(d), ctypes.byref(bd), plan._workspace.data_ptr(), g.data_ptr(),
               ctypes.byref(G1), ctypes.byref(G2), ptr(gmask))

        def shaped(buf, shape):
            if buf is None:
                return None
            lead = shape[0] if len(shape) == buf.dim() else 1
            if B > 1 and lead == 1:                           # shared by the whole batch: owns the sum over the materials
                folded = torch.empty((1,) + tuple(buf.shape[1:]), dtype=torch.float32, device=dev)
                launch(dev, N.lib().pbr_fold_gradient, buf.data_ptr(), folded.data_ptr(), B, buf.shape[1], H, W, 1, 1, 1)
                buf = folded
            return buf.reshape(shape)
        grads = [shaped(b, s) for b, s in zip(b1 + b2, ctx.shapes[:10])]
        return (None, *grads, shaped(gmask, ctx.shapes[10]))


def _blend_then_render_with_grad(albedo, normal, roughness, metallic, specular, *, blend, **kwargs):
    """Gradients that the fused backward kernel does not cover (view / light parameters through a blend, fp16; tiled maps where the fused
    tiled backward does not serve them):
    the same computation runs unfused through the differentiable pieces -- blend_maps (pbr_blend_maps + pbr_blend_maps_backward) for every map, the
    re-decode of the blended normal (decode_normal and its backward: base.py:191-242 runs again on assignment), then the
    evaluation with its backward kernel -- so a rendering loss on a blended material (example_blend.py:14-32 inside a
    training loop) reaches both materials, the mask and the light / view parameters."""
    from .blending import blend_maps
    if kwargs.get("out") is not None:
        raise NotImplementedError("gradients through the fused blend need out=None (the result must be a fresh tensor)")
    # tile=n (round 6): the blend and the re-decode are MAP-sized operations -- the reference blends, assigns, then repeats (base.py:524-537)
    # -- and the evaluation of the blended maps under tile=n is differentiable with map-sized (folded) gradients, so nothing here changes
    kwargs.pop("blend_flags", None)        # whole maps decide "already signed?" from their own values, as the reference does
    if kwargs.get("height_total") not in (None, albedo.shape[-2]):   # (the fused backward kernel takes row bands with given flags)
        # a ROW BAND cannot take that decision from its own rows (base.py:212 looks at the whole map), and the unfused
        # re-decode below has no way to be told the whole map's verdict
        raise NotImplementedError("gradients through a fused blend need the whole map, not a row band: blend the maps first "
                                  "(pypbr_amd.blending) and evaluate the blended material's bands")
    a2, n2, r2, m2, s2, mask = blend
    squeeze = albedo.dim() == 3

    def batched(t):
        return None if t is None else (t if t.dim() == 4 else t.unsqueeze(0))
    first = [batched(t) for t in (albedo, normal, roughness, metallic, specular)]
    second = [batched(t) for t in (a2, n2, r2, m2, s2)]
    k = batched(mask if mask.dim() != 2 else mask.unsqueeze(0))
    B = first[0].shape[0]

    def pick(t, b):
        return t[b if t.shape[0] > 1 else 0]
    outs = [[], [], [], [], []]
    for b in range(B):
        for i, (x, y) in enumerate(zip(first, second)):
            if x is None or y is None:
                outs[i].append(None)
                continue
            v = blend_maps(pick(x, b), pick(y, b), pick(k, b), is_normal=(i == 1))
            outs[i].append(decode_normal(v) if i == 1 else v)
    maps = [None if col[0] is None else torch.stack(col) for col in outs]
    if maps[3] is not None:
        maps[4] = None
    out = cook_torrance(*maps, **kwargs)
    return out[0] if squeeze else out


USE_TORCH_OPS = True       # tests flip this to compare the two bindings of the same C ABI


def _torch_op_can_take(albedo, kw) -> bool:
    """`torch.ops.pbr_hip.cook_torrance` (pypbr_amd/torch_ops.py) covers the plain evaluation; explicit output buffers,
    schedules, per-call tuning, autotuning and the fused blend stay on the ctypes plan."""
    if not isinstance(albedo, torch.Tensor) or not albedo.is_cuda or albedo.numel() == 0:      # zero-sized maps: RenderPlan.launch returns the empty image
        return False
    if kw.get("out") is not None or kw.get("blend") is not None or kw.get("autotune") or kw.get("tuning") or kw.get("schedule", N.SCHEDULE_AUTO) != N.SCHEDULE_AUTO:
        return False
    if kw.get("out_dtype") not in (None, torch.float32, torch.float16):
        return False
    if kw.get("view_type", "directional") != "directional":                 # the camera has no operator: the ctypes plan
        return False
    from . import torch_ops
    return torch_ops.available()


def _param_tensor(v, rows):
    """view / light / intensity for the operator: a tensor that requires grad goes in as it is (the operator's autograd
    formula returns its gradient); anything else as a small CPU tensor, device tensors through the cached host copy."""
    if isinstance(v, torch.Tensor):
        if (v.requires_grad and torch.is_grad_enabled()) or not v.is_cuda or DEVICE_PARAMETERS:
            return v                                         # device tensors: the operator reads them on the device (ABI 5)
        return torch.tensor(_host_vec3(v, rows=rows), dtype=torch.float32)
    t = torch.tensor(v, dtype=torch.float32)                 # Python numbers: no round trip (traceable by torch.compile)
    return t.reshape(3) if rows is None else t.reshape(-1, 3)


def _cook_torrance_via_torch_op(albedo, normal, roughness, metallic=None, specular=None, *, view_dir, light, light_intensity,
                                light_type="point", light_size=None, albedo_is_srgb=True, specular_is_srgb=True, return_srgb=True,
                                convert_to_diffuse_specular=False, y_offset=0, height_total=None, out_dtype=None, tile=1, rows=None,
                                out=None, schedule=N.SCHEDULE_AUTO, autotune=False, blend=None, blend_flags=None, tuning=None,
                                view_type="directional"):
    # (out / schedule / autotune / blend / view_type are at their defaults here -- _torch_op_can_take -- and named so that an unknown
    # keyword raises TypeError exactly as on the plan path; blend_flags without a blend means nothing on either path)
    lt = str(light_type).lower()
    if lt not in _LIGHT_TYPES:   # cooktorrance.py:62-65
        raise ValueError(f"Unsupported light_type: {lt}. Must be 'directional' or 'point'.")
    squeeze = albedo.dim() == 3
    a = _as_batched(albedo, (3,), "albedo")
    n = _as_batched(normal, (3,), "normal")
    r = _as_batched(roughness, (1,), "roughness")
    m = _as_batched(metallic, (1,), "metallic")
    s = _as_batched(specular, (3,), "specular")
    if m is None and s is None:                         # cooktorrance.py:115-118
        raise ValueError("Material must have either 'metallic' or 'specular' property.")
    if m is not None:
        s = None
    if out_dtype == torch.float16 and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (a, n, r, m, s)):
        raise NotImplementedError("gradients need a float32 result (fp16 maps are fine: their gradients come back in fp16)")
    ny, nx = tile_counts(tile)
    out = torch.ops.pbr_hip.cook_torrance(
        a, n, r, m, s, _param_tensor(view_dir, None), _param_tensor(light, -1), _param_tensor(light_intensity, -1),
        float(light_size) if light_size else 0.0, _LIGHT_TYPES[lt], bool(albedo_is_srgb), bool(specular_is_srgb),
        bool(convert_to_diffuse_specular), bool(return_srgb), int(y_offset), int(height_total or 0), ny, nx, int(rows or 0),
        out_dtype == torch.float16)
    return out[0] if squeeze else out


_PARAM_KEYS = ("view_dir", "light", "light_intensity")


def _param_grad(g: torch.Tensor, like, n_lights: int):
    """Shapes a [L,3] (or [3]) gradient like the parameter the caller passed: same shape, dtype and device; an intensity
    given once for several lights owns the sum."""
    if not isinstance(like, torch.Tensor) or not like.requires_grad:
        return None
    if g.dim() == 2 and like.numel() == 3 and n_lights > 1:
        g = g.sum(dim=0)
    return g.reshape(like.shape).to(device=like.device, dtype=like.dtype)


class _CookTorranceFn(torch.autograd.Function):
    """Autograd bridge: forward = the fused kernel, backward = pbr_cook_torrance_backward[_params] (one more streaming
    kernel that recomputes the forward terms).  Gradients flow to the maps and -- like the reference's autograd graph,
    cooktorrance.py:95-96, :126-140 -- to view_dir / light / light_intensity when those are tensors that require grad."""

    @staticmethod
    def forward(ctx, albedo, normal, roughness, metallic, specular, view_dir, light, light_intensity, kwargs):
        if kwargs.get("out") is not None:
            raise NotImplementedError("gradients need out=None (the result must be a fresh tensor)")
        if kwargs.get("blend") is not None:
            raise NotImplementedError("this autograd bridge takes no blend (functional.cook_torrance routes a blend under a gradient to _FusedBlendFn)")
        maps = (albedo, normal, roughness, metallic, specular)
        plan = plan_cook_torrance(*[None if t is None else t.detach() for t in maps], view_dir=view_dir, light=light,
                                  light_intensity=light_intensity, **kwargs)
        if plan.desc.out_dtype != N.F32:
            raise NotImplementedError("gradients need a float32 result (fp16 maps are fine: their gradients come back in fp16)")
        ctx.plan = plan
        ctx.in_shapes = [None if t is None else tuple(t.shape) for t in maps]
        ctx.params = (view_dir, light, light_intensity)
        ctx.save_for_backward(*[t for t in maps if t is not None])   # for autograd's in-place-modification check
        with torch.cuda.device(plan.device):
            result = plan.launch()
        plan.out = None          # backward recomputes; keeping the output in ctx would be a reference cycle
        return result

    @staticmethod
    def backward(ctx, grad_out):
        ctx.saved_tensors        # raises if a map was modified in place since forward (the kernel re-reads the maps)
        plan = ctx.plan
        d = plan.desc
        B, H, W = d.batch, d.height, d.width
        g = grad_out.reshape(B, 3, H, W).to(torch.float32).contiguous()
        channels = (3, 3, 1, 1, 3)
        present = (True, bool(d.normal.data), True, bool(d.metallic.data), bool(d.specular.data))
        gdtype = torch.float32 if d.map_dtype == N.F32 else torch.float16      # gradients in the maps' storage type
        want_params = any(ctx.needs_input_grad[5:8])
        wanted = [bool(ctx.needs_input_grad[i] and present[i] and ctx.in_shapes[i] is not None) for i in range(5)]
        tiled = bool(d.map_height) and (d.map_height, d.map_width) != (d.height_total, W)
        shared = [wanted[i] and B > 1 and (len(ctx.in_shapes[i]) == 3 or ctx.in_shapes[i][0] == 1) for i in range(5)]
        lib = N.lib()
        if tiled and not want_params and not any(shared):
            # MaterialBase.tile (base.py:524-537) under autograd: a texel owns the SUM over its repeats.  pbr_cook_torrance_backward_folded
            # hands out MAP-sized gradients -- one kernel that walks the maps and accumulates over the repeats in registers where it serves
            # the launch (one light, map rows of whole 4-texel groups), else backward + fold through its workspace
            h, w = d.map_height, d.map_width
            bufs = [torch.empty((B, channels[i], h, w), dtype=gdtype, device=g.device) if wanted[i] else None for i in range(5)]
            ws_bytes = lib.pbr_backward_folded_workspace_bytes(ctypes.byref(d))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g.device) if ws_bytes else None
            launch(g.device, lib.pbr_cook_torrance_backward_folded, ctypes.byref(d), g.data_ptr(), *[ptr(b) for b in bufs], ptr(ws))
            grads = [None if b is None else b.reshape(shape) for b, shape in zip(bufs, ctx.in_shapes)]
            return (*grads, None, None, None, None)
        bufs = [torch.empty((B, channels[i], H, W), dtype=gdtype, device=g.device) if wanted[i] else None for i in range(5)]
        ptrs = [ptr(b) for b in bufs]
        camera = plan.view_type == "point"                     # gp[0:3] is then the camera position's gradient (pbr_cook_torrance_camera_backward)
        if want_params:
            L = d.n_lights
            gp = torch.empty(3 + 6 * L, dtype=torch.float32, device=g.device)
            query = lib.pbr_camera_backward_workspace_bytes if camera else lib.pbr_param_grad_workspace_bytes
            ws = torch.empty(max(1, query(ctypes.byref(d)) // 4), dtype=torch.float32, device=g.device)
            launch(g.device, lib.pbr_cook_torrance_camera_backward if camera else lib.pbr_cook_torrance_backward_params, ctypes.byref(d),
                   g.data_ptr(), *ptrs, gp.data_ptr(), ws.data_ptr())
        elif camera:
            launch(g.device, lib.pbr_cook_torrance_camera_backward, ctypes.byref(d), g.data_ptr(), *ptrs, None, None)
        else:
            launch(g.device, lib.pbr_cook_torrance_backward, ctypes.byref(d), g.data_ptr(), *ptrs)
        grads = []
        for i, (b, shape) in enumerate(zip(bufs, ctx.in_shapes)):
            if b is None:
                grads.append(None)
                continue
            # a map repeated by a fused tile(), or shared by the whole batch, owns the SUM of the per-output-pixel gradients
            if tiled and H != d.height_total:
                raise NotImplementedError("gradients of a tiled evaluation with light / view gradients or batch-shared maps need the whole output, not a row band")
            if tiled or shared[i]:
                h, w = (d.map_height, d.map_width) if tiled else (H, W)
                folded = torch.empty((1 if shared[i] else B, b.shape[1], h, w), dtype=gdtype, device=b.device)
                launch(b.device, N.lib().pbr_fold_gradient_typed, b.data_ptr(), folded.data_ptr(), B, b.shape[1], h, w, H // h, W // w,
                       int(shared[i]), _DTYPES[gdtype])      # fp16 gradients: summed in fp32, rounded once
                b = folded
            grads.append(b.reshape(shape))
        pgrads = [None, None, None]
        if want_params:
            L = d.n_lights
            view, light, inten = ctx.params
            pgrads = [_param_grad(gp[0:3], view, 1) if ctx.needs_input_grad[5] else None,
                      _param_grad(gp[3:3 + 3 * L].reshape(L, 3), light, 1) if ctx.needs_input_grad[6] else None,
                      _param_grad(gp[3 + 3 * L:].reshape(L, 3), inten, L) if ctx.needs_input_grad[7] else None]
        return (*grads, *pgrads, None)


# ------------------------------------------------------------------ the rendering-loss step as one kernel
# The steps -- _MseStepFn (one image per material) and the six light-stack classes (a stack of L images under the orthographic view, one camera
# position or one position per shot; each as a step or, with the gradients of view / lights / intensities, a fit step) -- share one frame:
#   _shared_by_batch, _plain_kwargs   what the callers ask before they route a call to a step
#   _KINDS                            one row per kind of step: entry point, workspace query, fit / camera / per-shot / weighted
#   _step_plan, _launch_loss_step     plan without a result; targets, gradient buffers, loss, workspace and the ONE launch, by the kind's row
#   _keep_step, _kept_step            forward keeps the gradients in ctx; backward hands them over, or evaluates again when they are gone
#   _scale_step_gradients             the gradients times the upstream gradient of the loss, on the device
# A step class is its forward (which plan, which inputs are differentiable) and what its backward returns; the six stack classes come out of
# one factory (_stack_step_class), are chosen by one route (_route) and applied by one helper (_one_pass_loss).
class _StepNotServed(Exception):
    """pbr_cook_torrance_mse_step does not serve this descriptor as one pass (raised before anything is launched)."""


def _shared_by_batch(t, B: int) -> bool:
    """A map (or mask) that B > 1 materials share: it has no batch dimension, or one of size 1.  Its gradient is a sum over the batch, which
    the one-pass steps do not form."""
    return t is not None and B > 1 and (t.dim() < 4 or t.shape[0] == 1)


# what a keyword argument may be for a one-pass step to serve the call; anything else (an explicit result, a blend, a row band ...) is not plain
_PLAIN = {"out": (None,), "blend": (None,), "blend_flags": (None,), "rows": (None,), "height_total": (None,), "y_offset": (None, 0),
          "autotune": (None, False), "out_dtype": (None, torch.float32), "tile": (1, (1, 1))}


def _plain_kwargs(kw, excluded) -> bool:
    """The keyword arguments are plain for a one-pass step: each of the keys the caller excludes -- it drops them before it plans -- is absent
    or says nothing."""
    for k in excluded:
        if k in kw and kw[k] not in _PLAIN[k]:
            return False
    return True


_STEP_EXCLUDED = ("out", "blend", "out_dtype", "autotune", "rows")                       # rendering_loss_mse: tiles and row bands are the library's to answer
_STACK_EXCLUDED = _STEP_EXCLUDED + ("blend_flags", "height_total", "y_offset", "tile")   # light stacks: whole untiled maps


def _step_plan(maps, kwargs, params=None):
    """The plan of a loss step: the colours are never written."""
    if params is not None:
        kwargs = dict(kwargs, view_dir=params[0], light=params[1], light_intensity=params[2])
    plan = plan_cook_torrance(*[None if t is None else t.detach() for t in maps], **kwargs)
    plan.out = None
    return plan


# The step kinds, one row each.  The stack kinds take [B,L,3,H,W] targets.  fit: the entry point also leaves the parameter gradients.  camera:
# the plan has view_type="point" (the descriptor's view_dir is the camera's position).  per_shot: one camera position per shot -- the positions
# travel beside the plan, and a fit row is 9 L floats instead of 3 + 6 L.  weighted: a weight per pixel travels behind the targets.
_StepKind = collections.namedtuple("_StepKind", "entry query fit camera per_shot weighted")
_KINDS = {
    "step": _StepKind("pbr_cook_torrance_mse_step", "pbr_mse_step_workspace_bytes", False, False, False, False),
    "stack": _StepKind("pbr_cook_torrance_mse_stack_step", "pbr_mse_step_workspace_bytes", False, False, False, False),
    "fit": _StepKind("pbr_cook_torrance_mse_stack_fit_step", "pbr_mse_stack_fit_workspace_bytes", True, False, False, False),
    "camera_stack": _StepKind("pbr_cook_torrance_camera_mse_stack_step", "pbr_mse_step_workspace_bytes", False, True, False, False),
    "camera_fit": _StepKind("pbr_cook_torrance_camera_mse_stack_fit_step", "pbr_camera_mse_stack_fit_workspace_bytes", True, True, False, False),
    "view_stack": _StepKind("pbr_cook_torrance_view_mse_stack_step", "pbr_mse_step_workspace_bytes", False, True, True, False),
    "view_fit": _StepKind("pbr_cook_torrance_view_mse_stack_fit_step", "pbr_view_mse_stack_fit_workspace_bytes", True, True, True, False)}
# ... and the six stack kinds with a weight per pixel (kind + "_w"): the weighted entry point, the unweighted kind's workspace
_KINDS.update({k + "_w": r._replace(entry=r.entry.replace("mse_stack", "weighted_mse_stack"), weighted=True)
               for k, r in list(_KINDS.items()) if k != "step"})
# what the tests read, derived: kind -> (entry point, workspace query), and the kinds by column
_STEP_KINDS = {k: (r.entry, r.query) for k, r in _KINDS.items()}
_WEIGHTED_KINDS = tuple(k for k, r in _KINDS.items() if r.weighted)
_FIT_KINDS = tuple(k for k, r in _KINDS.items() if r.fit)
_VIEW_KINDS = tuple(k for k, r in _KINDS.items() if r.per_shot)
_POINT_KINDS = tuple(k for k, r in _KINDS.items() if r.camera and not r.per_shot) + _VIEW_KINDS


def _step_kind(kind, weights):
    """The kind a step class launches: its own, or its weighted sibling when the call carries weights."""
    return kind if weights is None else kind + "_w"


def _camera_rows(view_dir, L, device):
    """The L camera positions of a view-stack launch as the entry points take them: (host float[3 L], None) -- read now, at every call -- or
    (None, contiguous float32 [L,3] tensor on `device`) for positions that live on a ROCm device: the kernel reads them when it runs, nothing
    is copied to the host."""
    if isinstance(view_dir, torch.Tensor) and view_dir.is_cuda and DEVICE_PARAMETERS:
        c = view_dir.detach().to(device, torch.float32).reshape(L, 3).contiguous()
        if c.data_ptr() != view_dir.data_ptr():
            _warn_parameter_copy(view_dir, device)
        return None, c
    rows = _host_vec3(view_dir, rows=-1)
    if len(rows) != L:
        raise ValueError("view_dir holds %d positions for %d shots" % (len(rows), L))
    return (ctypes.c_float * (3 * L))(*[x for r in rows for x in r]), None


def _launch_loss_step(kind, plan, maps, targets, wanted, cameras=None, weights=None):
    """ONE launch of a loss step -> (gradient buffers | None per map, parameter gradients [3 + 6 L] | None, loss).  Raises _StepNotServed
    before anything is launched when the library does not serve the descriptor as one pass (e.g. tiled maps with several lights).
    `cameras`: the view kinds' [L,3] positions (the plan's own view is not read); their parameter gradients are [9 L].
    `weights`: the weighted kinds' per-pixel weights, in a shape `_stack_weights` accepts; brought to the maps' device as float32 like the
    targets (a copy for any other dtype or device) and handed over as a pointer and two strides in elements."""
    row = _KINDS[kind]
    if row.camera != (plan.view_type == "point"):
        raise ValueError("loss step %r does not take a plan with view_type=%r" % (kind, plan.view_type))
    d = plan.desc
    dev = plan.device                                       # the maps' device: targets handed over on the CPU, or on another GPU, are brought here
    lights = () if kind == "step" else (d.n_lights,)
    tgt = targets.detach().to(dev, torch.float32).reshape(d.batch, *lights, 3, d.height, d.width).contiguous()    # H x W: the OUTPUT (tiled maps: all repeats)
    gdtype = torch.float32 if d.map_dtype == N.F32 else torch.float16
    present = (True, bool(d.normal.data), True, bool(d.metallic.data), bool(d.specular.data))
    # in the map's OWN shape ([C,H,W] or [B,C,H,W]: the same memory layout), so that backward returns the buffer itself, not a view of
    # it -- autograd takes ownership of such a gradient instead of cloning it (a 4096^2 fp16 albedo: 73 us per step)
    bufs = [torch.empty(tuple(maps[i].shape), dtype=gdtype, device=dev) if wanted[i] and present[i] else None for i in range(5)]
    loss = torch.empty((), dtype=torch.float32, device=dev)
    gp = torch.empty(9 * d.n_lights if row.per_shot else 3 + 6 * d.n_lights, dtype=torch.float32, device=dev) if row.fit else None
    where = ()
    if row.per_shot:
        cam_host, cam_dev = _camera_rows(cameras, d.n_lights, dev)
        where = (cam_host, ptr(cam_dev))
    beside = ()
    if row.weighted:
        plane = d.height * d.width
        w = weights.detach().to(dev, torch.float32).reshape(d.batch, -1, d.height, d.width).contiguous()      # [B, L | 1, H, W]
        beside = (w.data_ptr(), w.shape[1] * plane, plane if w.shape[1] == d.n_lights else 0)
    lib = N.lib()
    ws_bytes = getattr(lib, row.query)(ctypes.byref(d))
    if ws_bytes == 0:
        raise _StepNotServed()
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)      # at least the bytes asked for, 8-byte aligned
    launch(dev, getattr(lib, row.entry), ctypes.byref(d), *where, tgt.data_ptr(), *beside, *[ptr(b) for b in bufs],
           *([] if gp is None else [gp.data_ptr()]), loss.data_ptr(), ws.data_ptr())
    if kind != "step":
        STACK_LAUNCHES[row.entry[len("pbr_cook_torrance_"):]] += 1
    return bufs, gp, loss


_NO_VIEW = (0.0, 0.0, 1.0)      # the view of a view-stack plan: never read (the positions come beside the descriptor)


def _plan_and_launch(kind, maps, kwargs, params, targets, wanted, weights=None):
    """_step_plan and _launch_loss_step for any kind.  The view kinds plan with a placeholder view and hand `params[0]`, the [L,3] positions,
    to the launch."""
    if _KINDS[kind].per_shot:
        plan = _step_plan(maps, kwargs, (_NO_VIEW, params[1], params[2]))
        return _launch_loss_step(kind, plan, maps, targets, wanted, cameras=params[0], weights=weights)
    return _launch_loss_step(kind, _step_plan(maps, kwargs, params), maps, targets, wanted, weights=weights)


def _keep_step(ctx, kind, maps, targets, kwargs, wanted, kept, params=None, weights=None):
    """Forward's bookkeeping: the gradients the launch left stay in ctx until backward hands them over.  The plan (descriptor + strong
    references to every map) is NOT kept: a second backward rebuilds it from the saved tensors -- the weights, saved next to the targets,
    among them."""
    ctx.kind, ctx.kwargs, ctx.wanted, ctx.grads, ctx.params = kind, kwargs, wanted, kept, params
    ctx.present = [t is not None for t in maps]
    ctx.save_for_backward(*[t for t in maps if t is not None], targets, *([] if weights is None else [weights]))


def _kept_step(ctx):
    """Backward's side: (gradient buffers, parameter gradients | None), given away -- autograd may keep the very buffers (e.g. as .grad).
    Differentiated again (retain_graph=True on the earlier backward) the first call gave them away, so the step is evaluated once more for
    fresh ones: the common single backward never pays for a copy."""
    saved = ctx.saved_tensors                               # in-place edits of the maps since forward are detected, as for any op
    kept, ctx.grads = ctx.grads, None
    if kept is None:
        it = iter(saved)
        maps = [next(it) if p else None for p in ctx.present]
        targets, weights = next(it), next(it, None)
        kept = _plan_and_launch(ctx.kind, maps, ctx.kwargs, ctx.params, targets, ctx.wanted, weights)[:2]
    return kept


def _scale_step_gradients(grads, grad_loss):
    """The gradients a loss step kept, times the upstream gradient of the loss, in place: ONE launch for all of them (they share a dtype and
    a device), on the device (pbr_scale_list_by_device_scalar: no host synchronisation, an early-out when the scalar is exactly 1)."""
    live = [b for b in grads if b is not None]
    if live:
        k = grad_loss.detach().to(live[0].device, torch.float32).reshape(1).contiguous()
        ptrs = (ctypes.c_void_p * len(live))(*[b.data_ptr() for b in live])
        counts = (ctypes.c_size_t * len(live))(*[b.numel() for b in live])
        launch(live[0].device, N.lib().pbr_scale_list_by_device_scalar, ptrs, counts, len(live), _DTYPES[live[0].dtype], k.data_ptr())


class _MseStepFn(torch.autograd.Function):
    """loss = mean((cook_torrance(maps) - target)^2) with its gradients from ONE kernel (pbr_cook_torrance_mse_step): forward
    evaluates, compares and differentiates in a single pass over the maps (32 + 12 bytes read, 32 written per pixel) and keeps
    the four gradients; backward hands them over, scaled by the upstream gradient on the device (no host synchronisation; a
    scalar of exactly 1 -- `loss.backward()` -- costs one early-out launch per map)."""

    # A training loop calls the step with the SAME leaf tensors every iteration (the optimiser updates them in place): the filled
    # descriptor of the last step is kept -- pointers, never values of maps -- keyed on the very tensors (weakly held: a dropped material
    # frees its maps), their addresses and shapes and the scalar arguments; light / view VALUES are re-read every call.  Small maps make the
    # step host-bound (150 us at 256^2 against 23 us captured into a graph); the descriptor is a third of that.
    _PLANS = collections.OrderedDict()
    _PLANS_MAX = 8
    _LOCK = threading.Lock()                                # guards _PLANS itself; a kept descriptor is refilled and launched under ITS entry's lock

    @staticmethod
    def _kept_plan(maps, kwargs):
        vals = tuple(host_values(kwargs.get(k)) for k in _PARAM_KEYS)
        rest = tuple(sorted((k, v if not isinstance(v, list) else tuple(v)) for k, v in kwargs.items() if k not in _PARAM_KEYS))
        try:
            hash(rest)
        except TypeError:
            return None, None, None
        # parameters on the device / with gradients: the general path every time; strided rows are evaluated through a copy (_as_batched):
        # nothing to keep
        if None in vals or any(t is not None and (t.stride(-1) != 1 or t.stride(-2) != t.shape[-1]) for t in maps):
            return None, None, None
        key = (tuple(None if t is None else (id(t), t.data_ptr(), tuple(t.shape), t.dtype) for t in maps), rest)
        hit = _MseStepFn._PLANS.get(key)
        if hit is not None:
            if hit.describes(maps):
                _MseStepFn._PLANS.move_to_end(key)
                return hit, key, vals                       # a KeptPlan: refreshed by the caller under the entry's lock
            del _MseStepFn._PLANS[key]
        return None, key, vals

    @staticmethod
    def forward(ctx, albedo, normal, roughness, metallic, specular, target, kwargs):
        maps = (albedo, normal, roughness, metallic, specular)
        # The process-wide lock covers the cache lookup and refill only: plan construction, the target's upload, the workspace
        # and the launch run outside it, under the ENTRY's own lock -- threads that drive different materials / GPUs do not serialise.
        with _MseStepFn._LOCK:
            hit, key, vals = _MseStepFn._kept_plan(maps, kwargs)
        plan = None
        if hit is not None and not hit.try_acquire():       # another thread is launching through this very plan: build a private one, keep nothing
            hit = key = None
        try:
            if hit is not None:
                if hit.refresh(vals):                       # light / view VALUES are re-read every call
                    plan = hit.plan
                else:                                       # another number of lights: another kernel, another plan
                    with _MseStepFn._LOCK:
                        if _MseStepFn._PLANS.get(key) is hit:
                            del _MseStepFn._PLANS[key]
            kept = plan is not None
            if plan is None:
                plan = _step_plan(maps, kwargs)
            wanted = [bool(ctx.needs_input_grad[i] and maps[i] is not None) for i in range(5)]
            try:
                bufs, _, loss = _launch_loss_step("step", plan, maps, target, wanted)
            except _StepNotServed:
                if kept:                                        # never again through the cache: the fallback must not meet it on every call
                    with _MseStepFn._LOCK:
                        _MseStepFn._PLANS.pop(key, None)
                raise
            entry = KeptPlan.adopt(plan, maps, vals) if not kept and key is not None else None
            if entry is not None:
                with _MseStepFn._LOCK:                          # cached only AFTER a launch that was served
                    _MseStepFn._PLANS[key] = entry
                    while len(_MseStepFn._PLANS) > _MseStepFn._PLANS_MAX:
                        _MseStepFn._PLANS.popitem(last=False)
        finally:
            if hit is not None:
                hit.release()
        _keep_step(ctx, "step", maps, target, kwargs, wanted, (bufs, None))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        grads, _ = _kept_step(ctx)
        _scale_step_gradients(grads, grad_loss)
        return (*grads, None, None)


def rendering_loss_mse(albedo: torch.Tensor, normal: Optional[torch.Tensor], roughness: torch.Tensor,
                       metallic: Optional[torch.Tensor] = None, specular: Optional[torch.Tensor] = None, *,
                       target: torch.Tensor, weights: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
    """`torch.nn.MSELoss()(cook_torrance(albedo, normal, roughness, metallic | specular, **kwargs), target)` -- the rendering loss of
    docs/source/tutorials/06_advanced.rst:73-107 for the predicted material -- as a 0-dim tensor on the maps' device.  When a map
    requires grad and the evaluation qualifies (whole untiled maps of the batch, fp32 result, light / view parameters without
    gradients, every map with its own planes) loss and gradients come out of ONE kernel, pbr_cook_torrance_mse_step; otherwise
    it is the differentiable evaluation followed by torch's MSE (same value to fp32 rounding, same gradients).  With view_type="point"
    (`view_dir` is the camera's position) and ONE light the call is the light stack of one image -- the same quantity: one image, its own
    clamp and encode, the mean over 3 B H W values -- and takes its one pass under `rendering_loss_mse_stack`'s conditions:
    pbr_cook_torrance_camera_mse_stack_step, or pbr_cook_torrance_camera_mse_stack_fit_step when `view_dir`, `light` or `light_intensity`
    requires grad; several lights summed into one image under the camera stay the composition.

    `weights` (optional): one weight per pixel, [1,H,W] / [B,1,H,W]; the loss is `(weights * (image - target) ** 2).mean()` over all 3 B H W
    elements.  With ONE light the call is `rendering_loss_mse_stack(weights=)` at L = 1 -- in both view types: its routes, its conversion of
    the weights (a copy for anything but float32 on the maps' device), its rules for zeros and NaNs; several lights summed into one image
    are the evaluation followed by the weighted mean.  `weights=None` goes where it went before."""
    maps = (albedo, normal, roughness, metallic, specular)
    params = tuple(kwargs.get(k) for k in _PARAM_KEYS)
    if weights is not None:
        if not isinstance(albedo, torch.Tensor) or albedo.dim() not in (3, 4) or not isinstance(target, torch.Tensor):
            raise ValueError("albedo must be [3,H,W] or [B,3,H,W], target a tensor")
        want = tuple(target.shape[:-3]) + (1,) + tuple(target.shape[-2:])
        if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != want or target.dim() != albedo.dim():
            raise ValueError("weights must be %s, got %s" % (want, tuple(weights.shape) if isinstance(weights, torch.Tensor) else type(weights)))
        if _one_light(params):                               # the stack of one image: the same quantity
            return rendering_loss_mse_stack(albedo, normal, roughness, metallic, specular, targets=target.unsqueeze(-4),
                                            weights=weights.unsqueeze(-4), **kwargs)
        return _weighted_mse(cook_torrance(albedo, normal, roughness, metallic, specular, **kwargs), target, weights)
    grad_maps = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in maps)
    grad_other = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in params + (target,))
    B = albedo.shape[0] if albedo.dim() == 4 else 1
    shared = B > 1 and any(_shared_by_batch(t, B) for t in maps)
    camera = _view_type(kwargs) == "point"
    if camera and torch.is_grad_enabled() and isinstance(target, torch.Tensor) and tuple(target.shape) == tuple(albedo.shape[:-3]) + (3,) + tuple(albedo.shape[-2:]):
        # one light: the L = 1 stack step (or fit step); several lights summed into one image have no fused camera form
        loss = _one_pass_loss(maps, params, target, kwargs) if _one_light(params) else None
        if loss is not None:
            return loss
    if grad_maps and not grad_other and _plain_kwargs(kwargs, _STEP_EXCLUDED) and not shared and albedo.is_cuda and not camera:
        # tiled maps (tile=n: MaterialBase.tile fused) take the one pass too -- the repeat-inner kernel leaves map-sized gradients -- where
        # the library serves them (one light, map rows of whole 4-texel groups); otherwise the three steps below
        kw = {k: v for k, v in kwargs.items() if k not in _STEP_EXCLUDED}
        try:
            return _MseStepFn.apply(albedo, normal, roughness, metallic, specular, target, kw)
        except _StepNotServed:
            pass
    out = cook_torrance(albedo, normal, roughness, metallic, specular, **kwargs)
    return torch.nn.functional.mse_loss(out.float(), target.to(out.device, torch.float32).reshape(out.shape))


# ------------------------------------------------------------------ light stacks: L images, one per light, out of one pass over the maps
# An extension over the reference (csrc/ct_stack.hip): a capture for SVBRDF fitting is a stack of photographs from ONE camera position with the
# light moved between the shots; image l of the stack is what `cook_torrance` gives for light l alone, and the loss is the MSE over all of them.
STACK_LAUNCHES = {"cook_torrance_stack": 0, "mse_stack_step": 0, "mse_stack_fit_step": 0,       # calls of the stack entry points (the tests count launches)
                  "camera_stack": 0, "camera_mse_stack_step": 0, "camera_mse_stack_fit_step": 0,     # ... and of their forms under the perspective camera
                  "view_stack": 0, "view_mse_stack_step": 0, "view_mse_stack_fit_step": 0,            # ... with one camera position per shot
                  "weighted_mse_stack_step": 0, "weighted_mse_stack_fit_step": 0,                     # ... and of the six loss steps with per-pixel weights
                  "camera_weighted_mse_stack_step": 0, "camera_weighted_mse_stack_fit_step": 0,
                  "view_weighted_mse_stack_step": 0, "view_weighted_mse_stack_fit_step": 0}


def _stack_lights(light, light_intensity) -> Tuple[int, int]:
    """(L, intensity rows) of a light stack, from shapes alone -- no device work, no read-back.  Raises ValueError for anything but
    1..MAX_LIGHTS lights of 3 components and 1 or L intensity rows."""
    def rows(v, name):
        n = v.numel() if isinstance(v, torch.Tensor) else torch.as_tensor(v, dtype=torch.float32).numel()
        if n == 0 or n % 3:
            raise ValueError("%s must be [3] or [L,3], got %d values" % (name, n))
        return n // 3
    L, R = rows(light, "light"), rows(light_intensity, "light_intensity")
    if L > N.MAX_LIGHTS:
        raise ValueError("a light stack holds between 1 and %d lights, got %d" % (N.MAX_LIGHTS, L))
    if R not in (1, L):
        raise ValueError("light_intensity must have 1 row or one per light (%d), got %d" % (L, R))
    return L, R


def _stack_views(view_dir, L: int) -> int:
    """Rows of a stack's `view_dir`, by element count, from shapes alone: 1 (3 values: one view for all shots) or L (3 L values: one per shot;
    for L = 1, [1,3] and [3] are the same thing).  Raises ValueError for anything else."""
    n = view_dir.numel() if isinstance(view_dir, torch.Tensor) else torch.as_tensor(view_dir, dtype=torch.float32).numel()
    if n == 3:
        return 1
    if n == 3 * L:
        return L
    raise ValueError("view_dir must be [3] (one view for all %d shots) or [L,3] = [%d,3] (one per shot), got %d values" % (L, L, n))


def _view_rows(view_dir):
    """`view_dir` [L,3] as something row l can be taken of (the composition hands row l to call l; a tensor keeps its graph)."""
    return (view_dir if isinstance(view_dir, torch.Tensor) else torch.as_tensor(view_dir, dtype=torch.float32)).reshape(-1, 3)


def _stack_plain(kw) -> bool:
    """The keyword arguments of a call that pbr_cook_torrance_stack / pbr_cook_torrance_mse_stack_step serve: whole untiled maps, a fresh fp32 result."""
    return _plain_kwargs(kw, _STACK_EXCLUDED)


def cook_torrance_stack(albedo: torch.Tensor, normal: Optional[torch.Tensor], roughness: torch.Tensor,
                        metallic: Optional[torch.Tensor] = None, specular: Optional[torch.Tensor] = None, *,
                        view_dir: TensorLike, light: TensorLike, light_intensity: TensorLike, **kwargs) -> torch.Tensor:
    """The L images of a light stack: `light` [L,3] (1 <= L <= 16, one light type, one view direction, one light_size), `light_intensity` [3] /
    [1,3] for all lights or [L,3]; image l is exactly `cook_torrance(..., light=light[l], light_intensity=light_intensity[l])`.  Returns
    [L,3,H,W], or [B,L,3,H,W] for batched maps, float32.  ONE launch (pbr_cook_torrance_stack: maps read and decoded once, the
    light-independent terms formed once per pixel) when nothing requires grad and the maps are whole and untiled; otherwise -- gradients, `tile`,
    `out_dtype` ... -- a torch.stack of L `cook_torrance` calls, differentiable like them.  With view_type="point" (`view_dir` is the camera's
    position) the one launch is pbr_cook_torrance_camera_stack, under the same conditions.  `view_dir` may also be [L,3], one view per shot
    (the rule is by element count: 3 values are one view for all shots): with view_type="point" one camera position per shot -- a handheld
    capture, camera and flash moving together -- and image l is `cook_torrance(view_dir=view_dir[l], light=light[l], ...)`, from ONE launch of
    pbr_cook_torrance_view_stack under the same conditions; with view_type="directional" one orthographic direction per shot, which has no
    kernel of its own and is always the torch.stack of L calls.  Other keyword arguments as for `cook_torrance`."""
    L, rows = _stack_lights(light, light_intensity)
    per_shot = _stack_views(view_dir, L) > 1
    if kwargs.get("out") is not None:
        raise ValueError("cook_torrance_stack allocates its result: out= is not supported")
    maps = (albedo, normal, roughness, metallic, specular)
    camera = _view_type(kwargs) == "point"
    if (_stack_plain(kwargs) and isinstance(albedo, torch.Tensor) and albedo.is_cuda and albedo.dim() in (3, 4) and albedo.numel() > 0
            and not _needs_grad(*maps, view_dir, light, light_intensity) and (camera or not per_shot)):
        kw = {k: v for k, v in kwargs.items() if k in ("light_type", "light_size", "albedo_is_srgb", "specular_is_srgb", "return_srgb",
                                                       "convert_to_diffuse_specular", "schedule", "tuning", "view_type")}
        B = 1 if albedo.dim() == 3 else albedo.shape[0]
        stack = torch.empty((B, L, 3) + tuple(albedo.shape[-2:]), dtype=torch.float32, device=albedo.device)
        # the plan describes ONE image per material; as `out` it gets the head of the stack's block -- contiguous, so the descriptor carries the
        # block's address and no strides -- and the stack's entry point spaces the materials 3 L planes apart itself
        plan = plan_cook_torrance(albedo, normal, roughness, metallic, specular, view_dir=_NO_VIEW if per_shot else view_dir, light=light,
                                  light_intensity=light_intensity, out=stack.view(B * L, 3, *stack.shape[-2:])[:B], **kw)
        if per_shot:
            cam_host, cam_dev = _camera_rows(view_dir, L, plan.device)
            launch(plan.device, N.lib().pbr_cook_torrance_view_stack, ctypes.byref(plan.desc), cam_host, ptr(cam_dev))
        else:
            launch(plan.device, N.lib().pbr_cook_torrance_camera_stack if camera else N.lib().pbr_cook_torrance_stack, ctypes.byref(plan.desc))
        STACK_LAUNCHES["view_stack" if per_shot else "camera_stack" if camera else "cook_torrance_stack"] += 1
        return stack[0] if albedo.dim() == 3 else stack
    lt = (light if isinstance(light, torch.Tensor) else torch.as_tensor(light, dtype=torch.float32)).reshape(-1, 3)
    it = (light_intensity if isinstance(light_intensity, torch.Tensor) else torch.as_tensor(light_intensity, dtype=torch.float32)).reshape(-1, 3)
    vt = _view_rows(view_dir) if per_shot else None
    images = [cook_torrance(albedo, normal, roughness, metallic, specular, view_dir=vt[l] if per_shot else view_dir, light=lt[l],
                            light_intensity=it[l if rows > 1 else 0], **kwargs) for l in range(L)]
    return torch.stack(images, dim=-4)


def _fit_step_backward(ctx, grad_loss):
    """What a fit step's backward returns (_MseStackFitFn, _CameraStackFitFn, _ViewStackFitFn): the kept map gradients and the block [view |
    lights L x 3 | intensities L x 3], both scaled by the upstream gradient on the device, the block sliced and shaped like the parameters.
    The first block -- 3 floats, or 3 L for the view kinds' per-shot positions -- is handed back as the entry point left it: the view
    direction's gradient behind its F.normalize Jacobian, or the camera positions' own."""
    grads, gp = _kept_step(ctx)
    _scale_step_gradients(grads, grad_loss)
    k = grad_loss.detach().to(gp.device, torch.float32).reshape(1).contiguous()
    launch(gp.device, N.lib().pbr_scale_by_device_scalar, gp.data_ptr(), gp.numel(), N.F32, k.data_ptr())
    per_shot = _KINDS[ctx.kind].per_shot
    L = gp.numel() // 9 if per_shot else (gp.numel() - 3) // 6
    first = 3 * L if per_shot else 3
    need = [ctx.needs_input_grad[5 + i] for i in range(3)]
    host = gp.cpu() if any(n and not p.is_cuda for n, p in zip(need, ctx.params)) else None      # ONE copy for every parameter held on the CPU

    def part(i, first, rows):
        if not need[i]:
            return None
        g = (gp if ctx.params[i].is_cuda else host)[first:first + 3 * rows]
        return _param_grad(g if i == 0 else g.reshape(rows, 3), ctx.params[i], L if i == 2 else 1)
    pgrads = [part(0, 0, first // 3), part(1, first, L), part(2, first + 3 * L, L)]
    return (*grads, *pgrads, None, None, None)


def _stack_step_class(name, kind, takes_params, fit, doc):
    """One of the six light-stack step classes: loss = mean(w (stack - targets)^2) with its gradients from ONE kernel, the entry point of `kind`
    (of its weighted sibling when the call carries weights: _step_kind).  Forward keeps the gradients, backward hands them over scaled by the
    upstream gradient on the device; a second backward evaluates again -- as _MseStepFn.  `apply(*maps, [view_dir, light, light_intensity,]
    targets, kwargs, weights)`: with `takes_params` the three parameters are inputs (else the plan reads them from `kwargs`), and with `fit`
    backward also returns their gradients (_fit_step_backward).  Built with type(), so that autograd names the node `<name>Backward`."""
    n_inputs = 8 if takes_params else 5

    def forward(ctx, *args):
        maps, params = args[:5], (args[5:8] if takes_params else None)
        targets, kwargs, weights = args[n_inputs:]
        launched = _step_kind(kind, weights)
        wanted = [bool(ctx.needs_input_grad[i] and maps[i] is not None) for i in range(5)]
        bufs, gp, loss = _plan_and_launch(launched, maps, kwargs, params, targets, wanted, weights)
        _keep_step(ctx, launched, maps, targets, kwargs, wanted, (bufs, gp), params, weights)
        return loss

    def backward(ctx, grad_loss):
        if fit:
            return _fit_step_backward(ctx, grad_loss)
        grads, _ = _kept_step(ctx)
        _scale_step_gradients(grads, grad_loss)
        return (*grads, *([None] * (n_inputs - 2)))

    cls = type(name, (torch.autograd.Function,), {"__doc__": doc, "forward": staticmethod(forward), "backward": staticmethod(backward)})
    cls.takes_params = takes_params
    return cls


_MseStackStepFn = _stack_step_class("_MseStackStepFn", "stack", False, False, """The orthographic stack step (pbr_cook_torrance_mse_stack_step): the
    gradients of the maps, summed over the lights, in 64 + 12 L bytes per pixel instead of L loss steps and autograd's accumulation.""")
_MseStackFitFn = _stack_step_class("_MseStackFitFn", "fit", True, True, """_MseStackStepFn with view_dir / light / light_intensity as differentiable
    inputs (pbr_cook_torrance_mse_stack_fit_step): the loss, the map gradients and the (3 + 6 L) gradients of view, lights and intensities -- a
    capture whose light positions, per-shot intensities or camera axis are fitted, with or without the maps.  Parameters that live on the device
    are read there (device_params): no read-back, so a whole step captures into a graph; a parameter held on the CPU receives a CPU gradient
    (one copy of the small block).""")
_CameraStackStepFn = _stack_step_class("_CameraStackStepFn", "camera_stack", False, False, """_MseStackStepFn under the perspective camera
    (view_type="point" in `kwargs`: `view_dir` is the camera's position): pbr_cook_torrance_camera_mse_stack_step.""")
_CameraStackFitFn = _stack_step_class("_CameraStackFitFn", "camera_fit", True, True, """_MseStackFitFn under the perspective camera
    (pbr_cook_torrance_camera_mse_stack_fit_step): the (3 + 6 L) gradients are the camera position's, the lights' and the intensities'.  The
    position's gradient is handed back as the kernel summed it (the per-pixel normalisation is differentiated in the kernel; there is no
    F.normalize of the position).""")
_ViewStackStepFn = _stack_step_class("_ViewStackStepFn", "view_stack", True, False, """_CameraStackStepFn with one camera position per shot
    (`view_dir` [L,3]): pbr_cook_torrance_view_mse_stack_step.  The positions, lights and intensities are inputs here (not differentiated:
    that is _ViewStackFitFn) because the positions travel beside the plan.""")
_ViewStackFitFn = _stack_step_class("_ViewStackFitFn", "view_fit", True, True, """_CameraStackFitFn with one camera position per shot
    (pbr_cook_torrance_view_mse_stack_fit_step): the 9 L gradients of the L positions, the lights and the intensities.  Positions on the device
    are read there at every launch; host positions are re-read at every call.""")
# (view type, one view per shot) -> (the step class, the fit class)
_STACK_CLASSES = {("directional", False): (_MseStackStepFn, _MseStackFitFn), ("point", False): (_CameraStackStepFn, _CameraStackFitFn),
                  ("point", True): (_ViewStackStepFn, _ViewStackFitFn)}


def _route(view_type, maps, params, targets, kwargs, on_device=None, weights=None):
    """Which one-pass form of the family `view_type` serves a stack-loss call: "fit" (the family's fit class: view, a light or an intensity
    requires grad, with or without the maps), "step" (its step class: only maps do) or None (the composition).  Both need the call's own view
    type to be the family's, plain arguments, untiled maps, every map with its own planes, targets that need no grad and maps on a ROCm device
    (`on_device`: None = ask the albedo).  No rule by L: both steps were ahead of the composition at every L measured, the single photograph
    included (profiles/light_stack_fit_step.json, camera_stack_probe.json).  `weights` do not change the answer -- "fit" and "step" are then
    the weighted siblings, _step_kind; ahead at every L measured in all three families (profiles/weighted_stack_probe.json) -- unless they
    require grad: the composition."""
    if view_type is not None and _view_type(kwargs) != view_type:      # None: the caller took the family from the call's own view type
        return None
    albedo = maps[0]
    B = albedo.shape[0] if albedo.dim() == 4 else 1
    shared = B > 1 and any(_shared_by_batch(t, B) for t in maps)
    if on_device is None:
        on_device = albedo.is_cuda
    if not on_device or shared or not _stack_plain(kwargs) or _needs_grad(targets, weights):
        return None
    if _needs_grad(*params):
        return "fit"
    return "step" if _needs_grad(*maps) else None


def _stack_route(maps, params, targets, kwargs, on_device=None, weights=None):
    """_route for the orthographic view: _MseStackFitFn, _MseStackStepFn or None."""
    return _route("directional", maps, params, targets, kwargs, on_device, weights)


def _camera_stack_route(maps, params, targets, kwargs, on_device=None, weights=None):
    """_route for view_type="point" (`view_dir` is the camera's position): _CameraStackFitFn, _CameraStackStepFn or None."""
    return _route("point", maps, params, targets, kwargs, on_device, weights)


_view_stack_route = _camera_stack_route      # `view_dir` [L,3], one position per shot (_ViewStackFitFn, _ViewStackStepFn): the camera stack's conditions


def _one_pass_loss(maps, params, targets, kwargs, per_shot=False, weights=None):
    """The loss from the one-pass class that serves the call -- the family by the call's view type and `per_shot`, "fit" or "step" by _route --
    or None: no route (one orthographic direction per shot has no kernel at all), or the library does not serve the descriptor as one pass.
    A class that takes the parameters as inputs gets them out of `kwargs`."""
    view_type = _view_type(kwargs)
    route = None if per_shot and view_type != "point" else _route(None, maps, params, targets, kwargs, None, weights)
    if route is None:
        return None
    cls = _STACK_CLASSES[view_type, per_shot][route == "fit"]
    dropped = _STACK_EXCLUDED + _PARAM_KEYS if cls.takes_params else _STACK_EXCLUDED
    kw = {k: v for k, v in kwargs.items() if k not in dropped}
    try:
        return cls.apply(*maps, *(params if cls.takes_params else ()), targets, kw, weights)
    except _StepNotServed:
        return None


def _one_light(params) -> bool:
    """The call's lights are ONE light with one intensity; whatever is wrong with them is the evaluation's to say."""
    try:
        return _stack_lights(params[1], params[2]) == (1, 1)
    except (ValueError, TypeError, AttributeError, RuntimeError):
        return False


def _stack_weights(weights, want) -> None:
    """Checks the per-pixel weights of a stack loss against the targets' shape `want` = ([B,] L, 3, H, W), from shapes alone: one plane per
    shot, ([B,] L, 1, H, W), or one plane for all shots, ([B,] 1, 1, H, W).  Raises ValueError for anything else."""
    per_shot = tuple(want[:-3]) + (1,) + tuple(want[-2:])
    shared = per_shot[:-4] + (1,) + per_shot[-3:]
    if not isinstance(weights, torch.Tensor) or tuple(weights.shape) not in (per_shot, shared):
        raise ValueError("weights must be %s (one plane per shot) or %s (one plane for all shots), got %s"
                         % (per_shot, shared, tuple(weights.shape) if isinstance(weights, torch.Tensor) else type(weights)))


def _weighted_mse(out, targets, weights):
    """mean(w (out - targets)^2) over all elements of `out`, `w` broadcast over the channels (and over the shots, for one plane): what the
    weighted steps compute, composed from torch ops -- differentiable in everything, the weights included."""
    d = out.float() - targets.to(out.device, torch.float32).reshape(out.shape)
    return (weights.to(out.device, torch.float32) * d * d).mean()


def rendering_loss_mse_stack(albedo: torch.Tensor, normal: Optional[torch.Tensor], roughness: torch.Tensor,
                             metallic: Optional[torch.Tensor] = None, specular: Optional[torch.Tensor] = None, *,
                             targets: torch.Tensor, weights: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
    """`torch.nn.MSELoss()(cook_torrance_stack(albedo, normal, roughness, metallic | specular, **kwargs), targets)`: the rendering loss over a
    stack of L photographs `targets` [L,3,H,W] / [B,L,3,H,W], as a 0-dim tensor on the maps' device; the gradient of each map is the sum over
    the lights.  ONE pass over the maps under the conditions `rendering_loss_mse` uses -- something requires grad, the targets do not, plain
    arguments, every map with its own planes, on a ROCm device -- and untiled maps: pbr_cook_torrance_mse_stack_step when only maps require
    grad, pbr_cook_torrance_mse_stack_fit_step when `view_dir`, `light` or `light_intensity` does (lights, per-shot intensities or the camera
    axis being fitted, with or without the maps: their gradients come out of the same pass; a [3] / [1,3] intensity owns the sum over the
    lights, a parameter on the CPU receives a CPU gradient).  With view_type="point" (`view_dir` is the camera's position) the two passes are
    pbr_cook_torrance_camera_mse_stack_step and pbr_cook_torrance_camera_mse_stack_fit_step under the same conditions, and the view's
    gradient is the position's.  `view_dir` [L,3] is one view per shot (`cook_torrance_stack`): with view_type="point" the two passes are
    pbr_cook_torrance_view_mse_stack_step and pbr_cook_torrance_view_mse_stack_fit_step, and the positions' gradient comes back [L,3] like
    the tensor passed; with view_type="directional" it is the composition.  Every other case (tiled maps, maps shared by the batch, targets
    that require grad, no gradients wanted) is the stack followed by torch's MSE: same value to fp32 rounding, same gradients.

    `weights` (optional) is one weight per pixel for a capture with a mask -- coverage that differs from shot to shot, clipped highlights,
    confidence: [L,1,H,W] / [B,L,1,H,W], one plane per shot, or [1,1,H,W] / [B,1,1,H,W], one plane for all shots, H and W the targets'.  The
    loss is then `(weights * (stack - targets) ** 2).mean()`, the weight broadcast over the three channels: the mean is still over all
    3 B L H W elements, the sum of the weights is not used (for the mean over valid pixels divide by the constant `weights.mean()`).  The
    one-pass routes are taken under the same conditions, through the weighted siblings of the six entry points
    (pbr_cook_torrance_weighted_mse_stack_step ...); weights that require grad take the composition, which honours them too.  The kernels
    read contiguous float32 weights on the maps' device: any other dtype (`bool` and `uint8` masks included) or device is converted with
    `.to(float32)` at every call, which is a copy.  No sign check: a negative weight is the caller's business.  A weight of exactly 0 beside
    a finite target and a finite render contributes exactly 0 to the loss and to every gradient; a NaN target under a zero weight still
    gives NaN (0 * NaN).  `weights=None` is the unweighted call in every respect."""
    L, _ = _stack_lights(kwargs.get("light"), kwargs.get("light_intensity"))
    per_shot = kwargs.get("view_dir") is not None and _stack_views(kwargs["view_dir"], L) > 1
    if not isinstance(albedo, torch.Tensor) or albedo.dim() not in (3, 4):
        raise ValueError("albedo must be [3,H,W] or [B,3,H,W]")
    ny, nx = tile_counts(kwargs.get("tile", 1))
    H = int(kwargs["rows"]) if kwargs.get("rows") is not None else ny * albedo.shape[-2] - (int(kwargs.get("y_offset") or 0) if (ny, nx) != (1, 1) else 0)
    want = ((L, 3, H, nx * albedo.shape[-1]) if albedo.dim() == 3 else (albedo.shape[0], L, 3, H, nx * albedo.shape[-1]))
    if not isinstance(targets, torch.Tensor) or tuple(targets.shape) != want:
        raise ValueError("targets must be the stack %s, got %s" % (want, tuple(targets.shape) if isinstance(targets, torch.Tensor) else type(targets)))
    if weights is not None:
        _stack_weights(weights, want)
    maps = (albedo, normal, roughness, metallic, specular)
    params = tuple(kwargs.get(k) for k in _PARAM_KEYS)
    loss = _one_pass_loss(maps, params, targets, kwargs, per_shot, weights)
    if loss is not None:
        return loss
    out = cook_torrance_stack(albedo, normal, roughness, metallic, specular, **kwargs)
    if weights is not None:
        return _weighted_mse(out, targets, weights)
    return torch.nn.functional.mse_loss(out.float(), targets.to(out.device, torch.float32))
