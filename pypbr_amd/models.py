"""`CookTorranceBRDF` with the reference's call signature, backed by one fused HIP kernel.

Reference: /root/reference/pypbr/models/cooktorrance.py (BRDFModel :27-30,
CookTorranceBRDF.__init__ :53-66, forward :68-182).  Same constructor, same
forward arguments, same exceptions; the ~130 ATen ops of the reference's forward are
replaced by a single call into libpbr_hip.so (pypbr_amd.functional.cook_torrance).
"""
import collections
import os
import weakref
from abc import ABC
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import _native
from . import functional as F_
from ._caches import KeptPlan, host_values, same_tensors, weak_refs
from .materials import MaterialBase, _normalised


# Device copies kept by `material.cache_on_device()` (see CookTorranceBRDF._staged): id(material) -> (weakref, bytes), least
# recently used first.  Together they stay below DEVICE_CACHE_CAP bytes (PBR_DEVICE_CACHE_CAP, default 4 GiB): a loop over a
# dataset of CPU materials evicts the oldest copies instead of growing until the device is full.
DEVICE_CACHE_CAP = int(os.environ.get("PBR_DEVICE_CACHE_CAP", str(4 << 30)))
_DEVICE_CACHES = collections.OrderedDict()


def _touch_device_cache(material):
    if id(material) in _DEVICE_CACHES:
        _DEVICE_CACHES.move_to_end(id(material))


def _register_device_cache(material, nbytes):
    _DEVICE_CACHES.pop(id(material), None)
    for key in [k for k, (ref, _) in _DEVICE_CACHES.items() if ref() is None or "_device_cache" not in ref().__dict__]:
        del _DEVICE_CACHES[key]
    _DEVICE_CACHES[id(material)] = (weakref.ref(material), nbytes)
    total = sum(n for _, n in _DEVICE_CACHES.values())
    while total > DEVICE_CACHE_CAP and len(_DEVICE_CACHES) > 1:
        _, (ref, n) = _DEVICE_CACHES.popitem(last=False)
        if ref() is not None:
            ref().__dict__.pop("_device_cache", None)
        total -= n


def _upload_together(tensors, compute):
    """Device copies of the tensors that are not on `compute` yet: the host-resident ones in ONE transfer (functional.upload_packed),
    tensors of another device one by one; `None` and tensors already there pass through."""
    host = [i for i, t in enumerate(tensors) if t is not None and t.device.type == "cpu"]
    moved = [None if t is None else (t if t.device == compute or t.device.type == "cpu" else t.to(compute)) for t in tensors]
    if host:
        views, _ = F_.upload_packed([tensors[i] for i in host], compute)
        for i, v in zip(host, views):
            moved[i] = v
    return tuple(moved)


class BRDFModel(nn.Module, ABC):
    """Abstract base class for BRDF models (cooktorrance.py:27-30)."""


class CookTorranceBRDF(BRDFModel):
    """Cook-Torrance BRDF: GGX distribution, Smith/Schlick-GGX geometry, Schlick
    Fresnel, Lambertian diffuse; directional or point light.

        brdf = CookTorranceBRDF(light_type="point")
        color = brdf(material, view_dir, light_dir_or_position, light_intensity, light_size)

    `view_type="point"` (an extension; keyword only, so that upstream's positional `override_device` keeps its place): the second argument of
    `forward` is the camera's POSITION, in the point light's coordinates, the way `light_dir_or_position` is a direction or a position by
    `light_type`; every pixel looks towards it (functional.cook_torrance, view_type).  The default, "directional", is upstream's one view
    direction for the whole image.
    """

    def __init__(self, light_type: str = "point", override_device: torch.device = None, *, view_type: str = "directional"):
        super().__init__()
        self.light_type = light_type.lower()
        if self.light_type not in ["directional", "point"]:
            raise ValueError(
                f"Unsupported light_type: {self.light_type}. Must be 'directional' or 'point'."
            )
        self.view_type = str(view_type).lower()
        if self.view_type not in ["directional", "point"]:
            raise ValueError(
                f"Unsupported view_type: {self.view_type}. Must be 'directional' or 'point'."
            )
        self.override_device = override_device

    @staticmethod
    def _staged(material, maps, blend, compute):
        """Device copies of maps that live elsewhere (CPU-resident materials: the reference's default, e.g.
        examples/example_brdf.py), in ONE allocation and ONE transfer (functional.upload_packed).  By default the maps are uploaded on every
        call -- the reference re-reads its maps every call too.  Opt-in (`material.cache_on_device()`, or
        functional.set_caching(device_maps=True) for every material): the copy is kept on the material, so a loop that
        evaluates an unchanged material again and again uploads it once (a 4096^2 material: 9.6 ms of PCIe per call
        otherwise).  The cache is keyed on the very tensor objects (held weakly) and their version counters:
        assigning a new map, or modifying one in place, uploads afresh; tensors without a version counter
        (torch.inference_mode) are never cached.  All cached copies together stay below DEVICE_CACHE_CAP bytes (least
        recently used first out).  Maps that carry a gradient are copied differentiably, uncached.
        `material.drop_device_cache()` frees the device copy."""
        tensors = tuple(maps) + tuple(blend or ())
        if any(t is not None and t.requires_grad for t in tensors):
            moved = tuple(None if t is None else t.to(compute) for t in tensors)
            return moved[:5], (None if blend is None else moved[5:])
        versions = tuple(None if t is None else F_.version_of(t) for t in tensors)
        wanted = (F_.CACHING["device_maps"] or material.__dict__.get("_cache_on_device", False))
        cacheable = wanted and all(v is not None for t, v in zip(tensors, versions) if t is not None)
        at, seen, refs, moved = (material.__dict__.get("_device_cache") if cacheable else None) or (None, None, (), None)
        if moved is not None and at == compute and seen == versions and same_tensors(refs, tensors):
            _touch_device_cache(material)
        else:
            moved = _upload_together(tensors, compute)
            if cacheable:
                material.__dict__["_device_cache"] = (compute, versions, weak_refs(tensors), moved)
                _register_device_cache(material, sum(t.numel() * t.element_size() for t in moved if t is not None))
        return moved[:5], (None if blend is None else moved[5:])

    # ---- plan reuse (round 5).  For small maps the call IS its host layer: at 256^2 the kernel takes 4.5 us, a graph
    # replay of the whole call 10 us, the eager call 22 us.  A device-resident material that is evaluated again keeps the filled C-ABI
    # descriptor of its last evaluation: the next call checks that it still describes the call -- the very map tensors (object, address,
    # shape), the flags, the light / view VALUES (host parameters are re-read every call: a CPU tensor edited in place is seen) --,
    # points it at a fresh result tensor and launches.  Only pointers are remembered, never values of maps: whatever is in the maps'
    # memory at launch time is what the kernel reads, exactly as without the cache.  Anything else (gradients, parameters on the device,
    # CPU-resident or pending maps, a lazy blend, another thread using the plan) takes the general path below.
    PLAN_REUSE = True

    def _reuse_plan(self, material, view_dir, light, intensity, light_size, return_srgb):
        d = material.__dict__
        store = d.get("_store")
        if store is None or d.get("_lazy_blend") is not None or d.get("_raw_normal") or self.override_device is not None:
            return None
        vals = (host_values(view_dir), host_values(light), host_values(intensity))
        if vals[0] is None or vals[1] is None or vals[2] is None:
            return None
        albedo, normal, rough = store.get("albedo"), store.get("normal", False), store.get("roughness")
        metallic = store.get("metallic")
        specular = store.get("specular") if metallic is None else None
        if (albedo is None or normal is False or rough is None or (metallic is None and specular is None) or not albedo.is_cuda
                or albedo.device != material.device):
            return None
        maps = (albedo, normal, rough, metallic, specular)     # the plan's own order (KeptPlan.adopt)
        grad = torch.is_grad_enabled()
        for t in maps:
            # rows must be dense: a map with strided rows is evaluated through a contiguous COPY (functional._as_batched), and a kept plan
            # would keep pointing at that copy while the caller edits the original
            if t is not None and (t.device != albedo.device or t.dtype.itemsize > 4 or not t.is_floating_point() or (grad and t.requires_grad)
                                  or t.stride(-1) != 1 or t.stride(-2) != t.shape[-1]):
                return None
        key = (self.light_type, light_size, bool(return_srgb), bool(material.albedo_is_srgb), bool(getattr(material, "specular_is_srgb", True)),
               d.get("_lazy_tile", (1, 1)),
               tuple((id(t), t.data_ptr(), t.shape, t.dtype, t.stride()) if t is not None else None for t in maps))
        kept_key, kept = d.get("_plan_cache") or (None, None)
        if kept is not None and (kept_key != key or not kept.describes(maps)):
            # the store moved on (resize, an assignment, to(), a conversion): the kept descriptor describes maps that are no longer the
            # material's.  It holds them only weakly, so nothing was pinned; drop it now rather than at the next refill.
            d.pop("_plan_cache", None)
            kept = None
        if kept is None:
            if d.get("_plan_seen") != key:                    # first sighting of this call: a material whose maps are new tensors every step
                d["_plan_seen"] = key                         # (a training loop) never pays for a plan it would not use twice
                return None
            return key
        if not kept.try_acquire():                            # another thread is launching through this plan right now
            return None
        plan = kept.plan
        try:
            if not kept.refresh(vals):
                return key                                    # another number of lights: another kernel, another plan
            dev = plan.device
            out = torch.empty(kept.out_shape, dtype=torch.float32, device=dev)
            plan.out = out                                    # for the duration of the launch only: the plan keeps no result alive
            plan.desc.out = out.data_ptr()
            if torch.cuda.current_device() == dev.index:
                plan.launch()
            else:
                with torch.cuda.device(dev):
                    plan.launch()
            return out[0] if plan._squeeze else out
        finally:
            plan.out = None
            kept.release()

    def forward(self, material, view_dir: Tensor, light_dir_or_position: Tensor, light_intensity: Tensor,
                light_size: Optional[float] = None, return_srgb: bool = True) -> Tensor:
        """Reflected colour, shape (3,H,W) -- or (B,3,H,W) for batched maps -- on
        `override_device or material.device`.

        Maps resident on a ROCm device are read in place.  Maps resident on the CPU
        (the reference's default, e.g. examples/example_brdf.py) are uploaded, evaluated
        on the device and the result is returned on the CPU; nothing is computed on the
        CPU.  `light_dir_or_position` / `light_intensity` may be (L,3) for L lights.
        """
        reuse_key = None
        if self.view_type == "point" and isinstance(material, MaterialBase):
            material.materialize_blend()                      # the camera renders real maps: a recorded blend or tile(n) is carried out first
            if material.lazy_tile != (1, 1):
                material.materialize_tile()
        if self.PLAN_REUSE and self.view_type != "point" and isinstance(material, MaterialBase):      # (a kept plan is an orthographic one)
            got = self._reuse_plan(material, view_dir, light_dir_or_position, light_intensity, light_size, return_srgb)
            if isinstance(got, torch.Tensor):
                return got
            reuse_key = got                                   # a tuple: the call qualifies, its plan is built below and kept
        out_device = _normalised(self.override_device or material.device)

        pending = material.__dict__.get("_lazy_blend")
        blend = None
        if pending is not None:
            # blending.blend_with_mask(..., lazy=True): both materials are complete (checked there); read the raw
            # stores so that nothing gets blended into a copy -- the fused kernel does it on the fly
            first, (second, mask) = material.__dict__["_store"], pending
            albedo, normal, roughness = first["albedo"], first["normal"], first["roughness"]
            metallic, specular = first.get("metallic"), None
            if metallic is None:
                specular = first["specular"]
            specular_is_srgb = bool(getattr(material, "specular_is_srgb", True))
            blend = (second["albedo"], second["normal"], second["roughness"], second.get("metallic") if metallic is not None else None,
                     second.get("specular") if metallic is None else None, mask)
        else:
            # attribute probes in the reference's order, so a material without a roughness /
            # normal entry raises the same AttributeError (cooktorrance.py:99-100).  A material of this
            # package is read through its raw store: attribute access would materialise a pending tile(n, lazy=True),
            # which this call hands to the kernel as wrap-around addressing instead.
            store = material.__dict__.get("_store") if isinstance(material, MaterialBase) else None
            if store is not None and material._has_pending():
                # maps nobody has seen yet (materials.py, _ingest: an image's samples, a normal map undecoded): the whole material goes up
                # in one transfer and becomes float / decoded on arrival; those forms stay the material's maps, the others are re-read
                # next call as ever
                store = {**store, **material._resident(keep=False)}

            def probe(name):
                if store is None:
                    return getattr(material, name)
                if name not in store:
                    raise AttributeError(f"'{type(material).__name__}' object has no attribute '{name}'")
                return store[name]

            def has(name):
                return (name in store) if store is not None else hasattr(material, name)

            roughness = probe("roughness")
            normal = probe("normal")
            metallic = specular = None
            specular_is_srgb = True
            if has("metallic") and probe("metallic") is not None:
                metallic = probe("metallic")
            elif has("specular") and probe("specular") is not None:
                specular = probe("specular")
                specular_is_srgb = bool(getattr(material, "specular_is_srgb", True))
            else:
                raise ValueError("Material must have either 'metallic' or 'specular' property.")
            albedo = store.get("albedo") if store is not None else material._maps.get("albedo")
            if albedo is None:
                raise AttributeError(f"'{type(material).__name__}' material has no albedo map")

        if out_device.type == "cuda":
            compute = out_device
        else:
            _native.require_device()
            compute = torch.device("cuda", torch.cuda.current_device())

        maps = (albedo, normal, roughness, metallic, specular)
        if any(t is not None and t.device != compute for t in maps + (blend or ())):
            maps, blend = self._staged(material, maps, blend, compute)
        kw = dict(view_dir=view_dir, light=light_dir_or_position, light_intensity=light_intensity, light_type=self.light_type,
                  light_size=light_size, albedo_is_srgb=bool(material.albedo_is_srgb), specular_is_srgb=specular_is_srgb,
                  return_srgb=return_srgb, tile=getattr(material, "lazy_tile", (1, 1)))
        if self.view_type != "directional":
            kw["view_type"] = self.view_type
        if reuse_key is not None and blend is None and albedo.numel() > 0:
            plan = F_.plan_cook_torrance(*maps, **kw)
            with torch.cuda.device(plan.device):
                color = plan.launch()
            kept = KeptPlan.adopt(plan, maps, (host_values(view_dir), host_values(light_dir_or_position), host_values(light_intensity)),
                                  tuple(plan.out.shape))
            if kept is not None:
                material.__dict__["_plan_cache"] = (reuse_key, kept)
            plan.out = None                                   # the result belongs to the caller; later calls bring their own
            return color
        color = F_.cook_torrance(*maps, blend=blend, **kw)
        if color.device == out_device:
            return color
        return F_.to_host(color, out_device) if out_device.type == "cpu" else color.to(out_device)
