"""Material containers with the surface the Cook-Torrance path reads.

Mirrors the part of pypbr.materials the hot path touches (SURVEY.md 8a rows H13-H16,
8b "Material surface"): the name -> tensor dict `_maps`, attribute access to maps,
`device`, `albedo_is_srgb` / `specular_is_srgb`, `linear_albedo` / `linear_specular`,
`to()`, `to_linear()` / `to_srgb()`, the two workflow conversions, `tile()`, the packed-tensor methods `from_tensor()` / `as_tensor()`.
Reference: /root/reference/pypbr/materials/{base,metallic,diffuse}.py.

Every computation (normal decode, colour transfer, workflow conversion) runs in
libpbr_hip.so on a ROCm device; with no device present those calls raise -- there is no
ATen/CPU arithmetic in this package.

Where the maps live.  A material's `device` is where its maps are HANDED OUT (the reference's
default: the CPU, e.g. examples/example_brdf.py).  Internally a map stays where it was last
produced: a CPU material's first whole-material operation (`resize`, `to_linear`, a workflow
conversion, a blend) uploads all its maps in ONE host-to-device copy (functional.upload_packed),
runs on the device and leaves the results THERE; later operations and `CookTorranceBRDF` read them
in place.  Only a caller that looks at a map (`material.albedo`, `_maps`, `as_dict()`, `clone()`,
`linear_albedo` ...) brings it home, once.  Round 3 staged every map through the device and back
per operation: load -> resize -> tile -> render was 5 x (H2D + launch + D2H) for the resize, the
same again for the normal decode, and one more upload of everything for the render
("What's missing" #3); now it is one upload and the download of the image.

Differences from the reference, all supersets:
  * maps may be any floating torch.Tensor on any device (the reference only files
    CPU float32 `torch.FloatTensor`s into `_maps`) and may carry a
    leading batch dimension [B,C,H,W] (F2).  A ROCm-resident tensor assigned to a material
    that still sits on its default device (cpu) pulls the MATERIAL onto the tensor's
    device instead of being copied to the host -- the rendering-loss loop of
    docs/source/tutorials/06_advanced.rst builds a material from predicted device tensors
    every step, and a silent device -> host -> device round trip of every map cost 9.8 ms
    per step at 2048^2 against 0.2 ms of kernels (tools/flow_trace.py);
  * `to_diffuse_specular_material(specular_is_srgb=...)` exposes the flag the upstream
    conversion forgets to set (F6); the default keeps upstream behaviour.
"""
import copy
import enum
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from . import functional as F_
from ._caches import VersionMemo


class NormalConvention(enum.Enum):
    """pypbr/utils/enums.py:12-14 (carried on materials; the BRDF never reads it)."""
    OPENGL = "opengl"
    DIRECTX = "directx"


def _is_image(value) -> bool:
    try:
        from PIL import Image
        return isinstance(value, Image.Image)
    except ImportError:  # pragma: no cover
        return False


def _is_map_value(value) -> bool:
    if value is None or isinstance(value, (np.ndarray, ImageMap)) or _is_image(value):
        return True
    return isinstance(value, torch.Tensor) and value.is_floating_point()


def _image_to_tensor(image, defer: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PIL image -> (C,H,W) float32 in [0,1] (base.py:143-164: 16-bit modes / 65535,
    mode F as is, RGBA -> RGB, everything else uint8 / 255).
    `defer=True`: 8- and 16-bit images come back as their own SAMPLES -- a (C,H,W) uint8 / uint16 view of PIL's (H,W,C) array, no
    transposing, no arithmetic -- and the division waits for `_samples_to_float` (host) or pbr_unpack_image (device).  `out`: a 1-D
    uint8 tensor of exactly the samples' size (the loader passes a slice of its page-locked block): the samples are put there."""
    if image.mode in ("I", "I;16", "I;16B", "I;16L", "I;16N"):
        arr = np.array(image, dtype=np.uint16)
        if defer:
            return _samples_tensor(arr, out)
        return (torch.from_numpy(arr.astype(np.float32)) / 65535.0).unsqueeze(0)
    if image.mode == "F":
        return torch.from_numpy(np.array(image, dtype=np.float32)).unsqueeze(0)
    if image.mode == "RGBA":
        image = image.convert("RGB")
    arr = np.array(image)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    if defer and arr.dtype == np.uint8:
        return _samples_tensor(arr, out)
    t = torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))
    return t.to(torch.float32).div(255) if t.dtype == torch.uint8 else t.to(torch.float32)


def _samples_tensor(arr: np.ndarray, out: Optional[torch.Tensor]) -> torch.Tensor:
    """(H,W) or (H,W,C) samples -> the (C,H,W) VIEW of them as a tensor; copied into `out` first when it has their size."""
    if out is not None and out.dtype == torch.uint8 and out.dim() == 1 and out.numel() == arr.nbytes and out.is_contiguous():
        np.copyto(out.numpy().view(arr.dtype).reshape(arr.shape), arr)
        t = out.view(torch.uint16 if arr.dtype == np.uint16 else torch.uint8).view(arr.shape)
    else:
        t = torch.from_numpy(arr)
    return t.unsqueeze(0) if t.dim() == 2 else t.permute(2, 0, 1)


def _samples_to_float(t: torch.Tensor) -> torch.Tensor:
    """The arithmetic `_image_to_tensor(image, defer=True)` left out, on the host, exactly as base.py:143-164 would have done it."""
    if t.dtype == torch.uint8:
        return t.contiguous().to(torch.float32).div(255)
    return t.to(torch.float32) / 65535.0


class ImageMap:
    """A PIL image the loader's worker threads already turned into a tensor (io.py): float (C,H,W), or -- conversion deferred --
    the image's samples (`_image_to_tensor(image, defer=True)`).  Filed into a material like the image itself."""
    __slots__ = ("tensor",)

    def __init__(self, tensor: torch.Tensor):
        self.tensor = tensor


# Whether maps that come from image files stay as SAMPLES (and a normal map undecoded) until the first operation that needs floats:
# None = when a ROCm device is there to do it on arrival; True / False force it (tests of the host side run with True).
DEFER_IMAGE_DECODE: Optional[bool] = None


def _defer_images() -> bool:
    return torch.cuda.is_available() if DEFER_IMAGE_DECODE is None else bool(DEFER_IMAGE_DECODE)


def _through_device(t: torch.Tensor, fn):
    """Runs a libpbr_hip op on `t`; CPU-resident maps are staged through the device."""
    if t.is_cuda:
        return fn(t)
    _native.require_device()
    res = fn(t.to("cuda"))
    if isinstance(res, tuple):
        return tuple(F_.to_host(r, t.device) for r in res)
    return F_.to_host(res, t.device)


def _normalised(device) -> torch.device:
    """torch.device("cuda") names the current device: spelled out, so that it compares equal to the tensors that live there."""
    device = device if isinstance(device, torch.device) else torch.device(device)
    if device.type == "cuda" and device.index is None and torch.cuda.is_available():
        return torch.device("cuda", torch.cuda.current_device())
    return device


def _compute_device(home) -> torch.device:
    """Where a material handed out on `home` is computed: `home` itself when it is a ROCm device, else the current one."""
    home = torch.device(home)
    if home.type == "cuda":
        return home
    _native.require_device()
    return torch.device("cuda", torch.cuda.current_device())


# "Already signed?" (base.py:212: `normal_map.min() < 0`) is a property of the tensor's VALUES, and for a signed map the
# reference returns the very tensor it was given.  The rendering-loss loop wraps the same decoded normal map in a new
# material every step; with functional.set_caching(decode_verdicts=True) the first decode of a tensor leaves its verdict
# in a 4-byte device flag, the second assignment of the same unchanged tensor (same object, same version counter) reads
# that flag once, and from then on a signed map is handed back as it is -- no kernel, no copy, the reference's object
# identity -- while an encoded map is decoded afresh.  Off by default: the version counter does not see every edit
# (functional.CACHING), and the reference looks at the values every time.
_DECODE_VERDICTS = VersionMemo()          # payload: [device flag, host verdict or None]


def _decode_remembering(t: torch.Tensor) -> torch.Tensor:
    ver = F_.version_of(t) if F_.CACHING["decode_verdicts"] else None
    if ver is None:                 # the default (functional.set_caching): decide afresh, on the device, every assignment
        return F_.decode_normal(t)
    hit = _DECODE_VERDICTS.get(t, ver)
    if hit is not None:
        if hit[1] is None:
            hit[1] = bool(hit[0].item())       # the decode that wrote it ran an assignment ago: no wait in practice
        if hit[1]:
            return t
        return F_.decode_normal(t)
    out, flag = F_._decode_normal_raw(t)
    _DECODE_VERDICTS.put(t, ver, [flag, None])
    return out


FIT_MAPS = ("albedo", "normal", "roughness", "metallic", "specular", "height")     # the maps of a fit: MaterialBase._fit_maps
_CALL_CACHES = ("_device_cache", "_plan_cache", "_plan_seen")     # what CookTorranceBRDF keeps in a material's __dict__ between calls


class MaterialBase:
    """Dynamic bag of texture maps (base.py:34-120)."""

    def __init__(self, albedo=None, albedo_is_srgb: bool = True, normal=None, roughness=None,
                 normal_convention: NormalConvention = NormalConvention.OPENGL,
                 device: torch.device = torch.device("cpu"), **kwargs):
        self.device = _normalised(device)
        self.normal_convention = normal_convention
        self._maps = {}
        self.albedo_is_srgb = albedo_is_srgb
        for name, value in (("albedo", albedo), ("normal", normal), ("roughness", roughness)):
            if value is not None:
                setattr(self, name, value)
        for name, value in kwargs.items():
            setattr(self, name, value)

    # -- attribute protocol: map-like values are filed in _maps, the rest are plain attributes
    def __setattr__(self, name, value):
        if name in ("albedo_is_srgb", "_maps", "device", "normal_convention", "specular_is_srgb"):
            object.__setattr__(self, name, value)
        elif _is_map_value(value):
            self.materialize_blend()                       # an assignment to a lazily blended material lands on blended maps
            if self.__dict__.get("_lazy_tile", (1, 1)) != (1, 1):
                self.materialize_tile()                    # ... and one to a material with a recorded tile(n) on REPEATED maps: the
                                                           # new map is not repeated again on read (base.py:524-537 tiles what is there)
            self._raw[name] = self._ingest(name, value)
        else:
            object.__setattr__(self, name, value)

    def __getattr__(self, name):
        d = self.__dict__
        pending = d.get("_lazy_blend")
        if name in d.get("_store", {}) or (pending is not None and name in pending[0]):   # a map only material 2 has
            return self._maps[name]       # anything but the BRDF sees blended, repeated maps at home (CookTorranceBRDF reads _store itself)
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")

    # `_maps` is the reference's name -> tensor dict: the PUBLIC view.  Reading it first resolves a pending lazy blend
    # (blending.blend_with_mask(..., lazy=True)) and a pending tile(n, lazy=True), decodes a normal map whose decode was
    # deferred, and brings every map that still sits on the compute device home to `self.device` -- whoever looks at the maps
    # sees what the reference's dict would hold.  The package's own code goes through `_raw` (the same dict, as it stands) and `_resident()`.
    @property
    def _maps(self):
        d = self.__dict__
        if d.get("_lazy_blend") is not None:
            self.materialize_blend()
        if d.get("_lazy_tile", (1, 1)) != (1, 1):
            self.materialize_tile()
        self._bring_home()
        return d.setdefault("_store", {})

    @_maps.setter
    def _maps(self, value):
        self.__dict__["_store"] = value

    @property
    def _raw(self) -> dict:
        """The name -> tensor dict as it stands: maps wherever they were last produced, a deferred normal still encoded."""
        return self.__dict__.setdefault("_store", {})

    def _is_away(self) -> bool:
        """A map of this material sits on another device than the one it is handed out on."""
        return any(t is not None and t.device != self.device for t in self._raw.values())

    def _has_pending(self) -> bool:
        """Some map is not yet what the reference's dict would hold: still an image's samples, or a normal map still undecoded."""
        return bool(self.__dict__.get("_raw_normal")) or any(F_.is_encoded(t) for t in self._raw.values())

    # -- what the fit path (losses.py, priors.py, optim.py) asks about the stored maps.  None of these reads `_maps`: no blend is carried
    # out, no tile is repeated, nothing is decoded or brought home.
    def _stored(self, names) -> list:
        """The stored maps under `names` as they stand, None for one that is absent."""
        store = self.__dict__.get("_store", {})
        return [store.get(k) for k in names]

    def _stores(self, name) -> bool:
        """A map is filed under `name` (whatever its state)."""
        return name in self.__dict__.get("_store", {})

    def _render_inputs(self) -> list:
        """Every value a rendering of this material depends on: the stored maps, a pending blend's second store and its mask (else None)."""
        other, mask = self.__dict__.get("_lazy_blend") or ({}, None)
        return list(self.__dict__.get("_store", {}).values()) + list(other.values()) + [mask]

    def _is_materialised(self, allow_tile: bool = False) -> bool:
        """The stored maps are the maps: no pending blend, nothing still encoded or undecoded, and no recorded tile(n) -- unless the
        caller evaluates the stored maps at every repeat itself (`allow_tile`)."""
        return self.__dict__.get("_lazy_blend") is None and (allow_tile or self.lazy_tile == (1, 1)) and not self._has_pending()

    def _fit_maps(self) -> dict:
        """name -> tensor of the stored floating-point maps a fit can optimise and regularise, in FIT_MAPS' order."""
        return {k: t for k, t in zip(FIT_MAPS, self._stored(FIT_MAPS)) if isinstance(t, torch.Tensor) and t.is_floating_point()}

    def _samples_on_host(self):
        """Maps that are still an image's samples become float32 where they are (the host): base.py:143-164's arithmetic."""
        store = self._raw
        for name, t in store.items():
            if F_.is_encoded(t):
                store[name] = _samples_to_float(t)

    def _bring_home(self):
        store, home = self._raw, self.device
        self._samples_on_host()
        if self.__dict__.get("_raw_normal"):
            self.__dict__["_raw_normal"] = False
            store["normal"] = self._process_normal_map(store["normal"])
        for name, t in store.items():
            if t is not None and t.device != home:
                store[name] = F_.to_host(t, home) if home.type == "cpu" else t.to(home)

    def _resident(self, keep: bool = True) -> dict:
        """name -> float tensor on the compute device for every map that is present.  Maps that are still on the host travel in ONE
        copy (functional.upload_packed): maps that are still an image's samples go as samples and become float32 on arrival, the
        normal map decoded in the same pass; a float normal map whose decode was deferred goes first, its decoded form written
        behind the others -- either way the material ends up as one dense block of planes.  `keep=True`: the device tensors become
        the material's maps (the operation that asked is about to replace them anyway); `keep=False` (CookTorranceBRDF): host maps
        stay the material's maps -- the reference re-reads them every call -- except maps nobody can have seen yet (samples, a
        deferred normal), whose float form on the device is the map from now on."""
        self.materialize_blend()
        d, store = self.__dict__, self._raw
        compute = _compute_device(self.device)
        names = [k for k, t in store.items() if t is not None]
        away = [k for k in names if store[k].device != compute]
        out = {k: store[k] for k in names}
        pending = bool(d.get("_raw_normal"))
        unseen = [k for k in away if F_.is_encoded(store[k])]
        if away:
            # only HOST maps ride the packed upload (its staging is a host memcpy); a map that requires grad takes the differentiable
            # copy, a map on ANOTHER GPU (material.to("cuda:1") from cuda:0) the device-to-device copy, ordered on its stream
            alone = [k for k in away if store[k].requires_grad or store[k].device.type != "cpu"]
            for k in alone:
                out[k] = store[k].to(compute)
            plain = [k for k in away if k not in alone]
            in_flight = pending and "normal" in plain
            as_samples = in_flight and F_.is_encoded(store["normal"])
            if in_flight and not as_samples:                     # raw float normal first: everything behind it is one dense block
                plain = ["normal"] + [k for k in plain if k != "normal"]
            if plain:
                views, block = F_.upload_packed([store[k] for k in plain], compute, tail_planes=3 if in_flight and not as_samples else 0,
                                                encoded_normal=plain.index("normal") if as_samples else None)
                out.update(zip(plain, views))
                if as_samples:
                    pending = False
                elif in_flight and block is not None:
                    out["normal"] = F_._decode_normal_raw(out["normal"], out=block[-3:])[0]
                    pending = False
        if pending:
            out["normal"] = F_.decode_normal(out["normal"])
        if d.get("_raw_normal"):
            d["_raw_normal"] = False
            store["normal"] = out["normal"]
        for k in (away if keep else unseen):
            store[k] = out[k]
        return out

    def materialize_blend(self):
        """Carries out a pending lazy blend: the maps become real blended tensors (blend.hip kernels)."""
        pending = self.__dict__.get("_lazy_blend")
        if pending is not None:
            from .blending import _blend_dicts
            self.__dict__["_lazy_blend"] = None
            other, mask = pending
            store = self.__dict__["_store"]
            for name, result in _blend_dicts(dict(store), other, mask).items():
                store[name] = self._settle(name, result)      # normals pass through _process_normal_map, as upstream
        return self

    def _settle(self, name, t):
        """A map PRODUCED by this package (a blend, a conversion) becomes the material's: it stays on the device it was computed on,
        a normal map passes through _process_normal_map as on any assignment upstream."""
        if t is None:
            return None
        if name == "normal":
            return self._process_normal_map(t)
        return t

    def _ingest(self, name, value):
        if value is None:
            return None
        fresh = False                                # nobody else holds the tensor: its decode may wait for the first device operation
        if isinstance(value, torch.Tensor):
            if value.is_cuda and self.device.type == "cpu":
                self.device = value.device           # a device tensor pulls the material onto its device (module docstring)
            t = value.to(self.device)
        elif isinstance(value, np.ndarray):
            t = torch.from_numpy(value).float().to(self.device)
        elif _is_image(value) or isinstance(value, ImageMap):
            # base.py:143-164 converts and base.py:191-242 decodes at assignment.  A map that comes out of an image file lives on the
            # host and nobody can look at it but through this material: it is stored as loaded -- the image's own samples, a normal map
            # undecoded -- and becomes float32 on the device together with the first operation that uploads the material (a quarter of
            # the bytes on the way, no conversion on the host), or on the host when somebody reads it first.
            fresh = self.device.type == "cpu" and _defer_images()
            t = value.tensor if isinstance(value, ImageMap) else _image_to_tensor(value, defer=fresh)
            if F_.is_encoded(t) and not fresh:
                t = _samples_to_float(t)
            fresh = fresh and t.dim() == 3
            if not F_.is_encoded(t):
                t = t.to(self.device)
        else:  # pragma: no cover  (guarded by _is_map_value)
            raise TypeError(f"Unsupported image type: {type(value)}. Supported types are PIL.Image.Image, "
                            "np.ndarray, and torch.FloatTensor.")
        if name == "normal":
            self.__dict__["_raw_normal"] = False
            if fresh:
                if t.shape[0] not in (2, 3):
                    raise ValueError("Normal map must have 2 or 3 channels.")
                self.__dict__["_raw_normal"] = True
                return t
            return self._process_normal_map(t)
        return t

    @staticmethod
    def _process_normal_map(normal_map: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """base.py:191-242 on the device; a batch is decoded map by map (the "already
        signed?" test of :212 is per map)."""
        if normal_map is None:
            return None
        if normal_map.shape[-3] not in (2, 3):
            raise ValueError("Normal map must have 2 or 3 channels.")
        if normal_map.dim() == 4:
            return torch.stack([_through_device(n, F_.decode_normal) for n in normal_map], dim=0)
        if (normal_map.is_cuda and not normal_map.requires_grad and normal_map.dim() == 3 and normal_map.shape[0] == 3
                and normal_map.is_contiguous() and normal_map.dtype in (torch.float32, torch.float16)):
            return _decode_remembering(normal_map)
        return _through_device(normal_map, F_.decode_normal)

    # -- device management (base.py:245-259)
    def to(self, device):
        """base.py:245-259.  Moving to a ROCm device takes ONE host-to-device copy of all maps into one allocation
        (functional.upload_packed): a launch streams every plane of the material at once, and planes that share an allocation stay
        close together in the address space (1-6 % faster and steadier than maps scattered over the heap)."""
        self.device = _normalised(device)
        self.materialize_blend()
        if self.device.type == "cuda":
            self._resident(keep=True)
        else:
            self._bring_home()
        return self

    def _bring_home_normal(self):
        self.__dict__["_raw_normal"] = False
        self._raw["normal"] = self._process_normal_map(self._raw["normal"])

    # -- properties
    @property
    def linear_albedo(self):
        """base.py:262-277: a fresh linear copy when the stored map is sRGB."""
        albedo = self._maps.get("albedo")
        if albedo is None:
            return None
        return _through_device(albedo, F_.srgb_to_linear) if self.albedo_is_srgb else albedo

    @property
    def size(self) -> Optional[Tuple[int, int]]:
        """(height, width) of the first map that is present (base.py:293-307)."""
        ny, nx = self.lazy_tile
        for t in self.__dict__.get("_store", {}).values():       # a pending blend does not change the size
            if t is not None:
                return (t.shape[-2] * ny, t.shape[-1] * nx)
        return None

    def as_dict(self):
        self.materialize_tile()
        return dict(self._maps)

    # -- export (base.py:781-878): the way out of the package.  The quantisation runs on the device, csrc/pack_image.hip
    def to_numpy(self):
        """base.py:781-791: name -> the float map as a numpy array (None stays None)."""
        return {name: (None if t is None else t.cpu().numpy()) for name, t in self.as_dict().items()}

    def to_pil(self, maps_mode=None):
        """base.py:793-850: name -> PIL.Image (None stays None), in the maps' dict order.  Default modes are torchvision's to_pil_image
        of the float map -- `mul(255).byte()`, 3 channels RGB, anything else L --; a map whose entry in `maps_mode` is a 16-bit mode
        ("I", "I;16", "I;16B", "I;16L", "I;16N") becomes mode I;16 by (t * 65535).clip(0, 65535).astype(uint16); any other requested
        mode is ignored, as upstream; the normal map passes through (n + 1.0) * 0.5 first.  A 16-bit mode on a map of more than one
        channel raises ValueError (upstream fails inside PIL).

        The samples are made ON THE DEVICE by one pbr_pack_images launch per map size and come home in one copy of a quarter (half) of
        the float bytes (functional.download_samples); the images are built over that block, no arithmetic on the host.  A pending
        lazy blend or tile is carried out first, as for as_dict.  Maps that live on the device stay there: the stored tensors are the
        same objects afterwards.  A CPU-home map that is STILL an image's samples, asked for in its own width, is handed back as those
        samples with no device work ((k / 255) * 255 truncates back to k for every k, and likewise for 65535: exact); the normal map
        never is -- decode and encode do not round-trip, upstream's neither.  Outside [0, 1] the samples saturate and NaN gives 0
        (numerical differences)."""
        from PIL import Image
        modes = {} if maps_mode is None else maps_mode
        self.materialize_tile()
        self.materialize_blend()
        store, d = self._raw, self.__dict__
        wide, direct, through = {}, {}, []
        for name, t in store.items():
            if t is None:
                continue
            if t.dim() != 3:
                raise ValueError("to_pil takes (C,H,W) maps; map '%s' is %s" % (name, tuple(t.shape)))
            channels = 3 if name == "normal" and d.get("_raw_normal") else t.shape[0]
            wide[name] = modes.get(name, "RGB") in ("I", "I;16", "I;16B", "I;16L", "I;16N")
            if wide[name] and channels != 1:
                raise ValueError("Map '%s' has %d channels: a 16-bit mode takes a map of one channel." % (name, channels))
            if name == "normal" and channels != 3:
                raise ValueError("to_pil takes a normal map of 3 channels, got %d" % channels)
            if F_.is_encoded(t) and name != "normal" and t.element_size() == (2 if wide[name] else 1):
                direct[name] = t.permute(1, 2, 0).numpy()                 # PIL's own (H,W,C) array again
            else:
                through.append(name)
        samples = dict(direct)
        if through:
            maps = self._resident(keep=False)
            samples.update(F_.download_samples({k: maps[k] for k in through}, {k: 16 if wide[k] else 8 for k in through}))
        images = {}
        for name, t in store.items():
            if t is None:
                images[name] = None
                continue
            a = samples[name]
            if a.shape[2] == 1:
                images[name] = Image.fromarray(a[:, :, 0])                # uint8 -> L, uint16 -> I;16
            elif a.shape[2] == 3:
                images[name] = Image.fromarray(a)                         # RGB
            else:
                images[name] = Image.fromarray(a).convert("L")            # upstream: 2 channels LA, 4 RGBA, then convert("L")
        return images

    def save_to_folder(self, folder_path: str):
        """base.py:869-878: every map that is present as <name>.png under `folder_path` (io.save_material_to_folder)."""
        from .io import save_material_to_folder
        save_material_to_folder(self, folder_path)

    @property
    def normal_rgb(self):
        """base.py:279-291: the normal map as colours, (normal + 1) * 0.5, or None -- one affine pass of csrc/packing.hip (n * 0.5 + 0.5
        rounds once, to the same float)."""
        normal = self._maps.get("normal")
        if normal is None:
            return None
        return _through_device(normal, lambda t: F_._pack([t], [None], [(0.5, 0.5)]))

    # -- packed tensors (base.py:319-487); csrc/packing.hip: one launch each way, forward and backward
    def as_tensor(self, names=None, normalize: bool = False) -> torch.Tensor:
        """base.py:319-414: the selected maps stacked along the channels, on the material's device.  `names`: None or empty = every map
        in dict order; else a list of map names and (name, channel_limit) tuples.  `normalize`: every map but the normal map as
        (t - 0.5) / 0.5.  Upstream's errors, raised before any device work.  It stacks what a reader of `_maps` would see: a pending
        lazy blend or tile is carried out, a deferred normal decode too.  ONE launch writes the result (functional.pack_planes)."""
        selected = []
        if names:
            if not isinstance(names, list):
                raise TypeError("names must be a list of strings or tuples.")
            for item in names:
                if isinstance(item, str):
                    selected.append((item, None))
                elif isinstance(item, tuple):
                    if len(item) != 2:
                        raise ValueError("Each tuple in names must have exactly two elements: (map_name, channel_limit).")
                    map_name, channel_limit = item
                    if not isinstance(map_name, str):
                        raise TypeError("The first element of each tuple must be a string (map name).")
                    if not isinstance(channel_limit, int) or channel_limit <= 0:
                        raise ValueError("The second element of each tuple must be a positive integer (channel limit).")
                    selected.append((map_name, channel_limit))
                else:
                    raise TypeError("Each item in names must be either a string or a tuple of (str, int).")
        self.materialize_blend()                                 # the names and channel counts of a pending blend are the blended maps'
        store = self._raw
        if not names:
            selected = [(name, None) for name in store.keys()]
        shapes = []
        for name, channel_limit in selected:
            if name not in store:
                raise KeyError(f"Map '{name}' does not exist in the texture maps.")
            t = store[name]
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"Map '{name}' is not a torch.Tensor.")
            available = 3 if name == "normal" and self.__dict__.get("_raw_normal") else t.shape[-3]     # a deferred decode gives 3
            if channel_limit is not None and channel_limit > available:
                raise ValueError(f"Requested {channel_limit} channels for map '{name}', but only {available} channels are available.")
            shapes.append(tuple(t.shape[:-3]) + tuple(t.shape[-2:]))
        if not selected:
            raise ValueError("No valid texture maps found to stack.")
        if not all(s == shapes[0] for s in shapes):
            raise ValueError("All texture maps must have the same spatial dimensions for concatenation.")
        self.materialize_tile()
        maps = self._resident(keep=True)
        ts = [maps[name] for name, _ in selected]
        dtype = ts[0].dtype
        for t in ts[1:]:
            dtype = torch.promote_types(dtype, t.dtype)
        out = F_.pack_planes([t.to(dtype) for t in ts], [limit for _, limit in selected],
                             [bool(normalize) and name != "normal" for name, _ in selected])
        if out.device != self.device:
            out = F_.to_host(out, self.device) if self.device.type == "cpu" else out.to(self.device)
        return out

    @classmethod
    def from_tensor(cls, tensor: torch.Tensor, names=None, normal_convention: NormalConvention = NormalConvention.OPENGL,
                    is_normalized: bool = False, device: torch.device = torch.device("cpu")):
        """base.py:416-487: a material of this class from a packed (C_total,H,W) tensor -- (B,C_total,H,W) too -- and `names` =
        [(map_name, channels), ...].  Every map is its channels (x 0.5 + 0.5 when `is_normalized`); a 2-channel "normal" gets its z
        and is normalised; a 3-channel "normal" is stored AS GIVEN, as upstream stores it (no decode: under `is_normalized` it ends up
        in [0, 1]).  Upstream's configuration errors, raised before any device work.  ONE launch writes all maps into one
        allocation (functional.unpack_planes): they are new tensors, never views of `tensor`, and stay on the compute device -- a device
        tensor puts the material on its device, for a CPU tensor `device` is where the maps are handed out.  Differentiable."""
        instance = cls(normal_convention=normal_convention, device=device)
        if not names:
            names = []                                           # upstream: the maps of a fresh instance -- none
        config, total = [], 0
        for item in names:
            if isinstance(item, str):                            # upstream infers the count from the instance's map: a fresh one has none
                raise KeyError(f"Cannot infer channel count for map '{item}'. Provide a tuple instead.")
            elif isinstance(item, tuple):
                if len(item) != 2:
                    raise ValueError("Each tuple must be (map_name, channel_limit).")
                config.append((item[0], item[1]))
                total += item[1]
            else:
                raise TypeError("Configuration items must be a string or tuple (str, int).")
        if not isinstance(tensor, torch.Tensor) or tensor.dim() not in (3, 4):
            raise ValueError("a packed tensor is (C,H,W) or (B,C,H,W), got %s" % (tuple(tensor.shape) if isinstance(tensor, torch.Tensor) else type(tensor),))
        channels = tensor.shape[-3]
        if channels != total:
            raise ValueError(f"Packed tensor has {channels} channels, but configuration expects {total} channels.")
        if not config:
            return instance
        if tensor.dtype not in (torch.float32, torch.float16):
            raise TypeError("from_tensor supports float32/float16, got %s" % tensor.dtype)
        if any(not isinstance(n, int) or n < 1 for _, n in config):
            raise ValueError("a map of a packed tensor has at least one channel, got %s" % (config,))
        if tensor.is_cuda and instance.device.type == "cpu":
            instance.device = tensor.device                      # a device tensor pulls the material onto its device (module docstring)
        t = tensor if tensor.is_cuda else tensor.to(_compute_device(instance.device))
        for (name, _), m in zip(config, F_.unpack_planes(t, config, is_normalized=is_normalized)):
            instance._raw[name] = m                              # upstream writes _maps directly: no _process_normal_map
            if name == "normal":
                instance.__dict__["_raw_normal"] = False
        return instance

    def cache_on_device(self, enable: bool = True):
        """Opt-in: CookTorranceBRDF keeps the device copy of this CPU-resident material between calls (one upload for a
        loop over an unchanged material instead of one per call: 9.6 ms for a 4096^2 material).  The copy is recognised
        as current by tensor identity and version counter, which do not see `.data` edits or edits of a numpy array that
        shares a map's memory -- hence opt-in (functional.set_caching(device_maps=True) turns it on for every material).
        All cached copies together are bounded (models.DEVICE_CACHE_CAP, least recently used evicted first)."""
        object.__setattr__(self, "_cache_on_device", bool(enable))
        if not enable:
            self.drop_device_cache()
        return self

    def drop_device_cache(self):
        """Frees the device copy CookTorranceBRDF keeps of a CPU-resident material between calls."""
        return self._drop_call_caches(("_device_cache",))

    def _drop_call_caches(self, keys=_CALL_CACHES):
        """Forgets what CookTorranceBRDF keeps on a material between calls: it describes the tensors of the material it was made for."""
        for k in keys:
            self.__dict__.pop(k, None)
        return self

    def _convert_in_place(self, name, flag, fn):
        """One map through a colour transfer, on the device, the result left there (module docstring)."""
        if self._raw.get(name) is not None:
            self._raw[name] = fn(self._resident(keep=True)[name])

    # -- colour space, in place, returning self (base.py:754-778)
    def to_linear(self):
        self.materialize_blend()
        if self._raw.get("albedo") is not None and self.albedo_is_srgb:
            self._convert_in_place("albedo", "albedo_is_srgb", F_.srgb_to_linear)
            self.albedo_is_srgb = False
        return self

    def to_srgb(self):
        self.materialize_blend()
        if self._raw.get("albedo") is not None and not self.albedo_is_srgb:
            self._convert_in_place("albedo", "albedo_is_srgb", F_.linear_to_srgb)
            self.albedo_is_srgb = True
        return self

    # -- normal-map operations (base.py:673-729), returning self; csrc/normal_ops.hip.  The new normal map is stored as it comes out of the
    # kernel, never through _settle / _process_normal_map (upstream writes _maps["normal"] directly: a flat height's (0, 0, 1) has no
    # negative value, and the "already signed?" decode would turn it into (-1, -1, 1) / sqrt(3)); it stays on the compute device.
    def invert_normal(self):
        """base.py:673-687: y of the normal map negated (no renormalisation) and normal_convention swapped -- the swap happens
        with no normal map too."""
        self.materialize_blend()
        if self._raw.get("normal") is not None:
            n = self._resident(keep=True)["normal"]
            in_place = not (n.requires_grad and torch.is_grad_enabled()) and F_._rows_dense(n) is n    # as upstream's utils.invert_normal
            self._raw["normal"] = F_.transform_normals(n, ((1.0, 0.0), (0.0, -1.0)), False, out=n if in_place else None)
        self.normal_convention = (NormalConvention.DIRECTX if self.normal_convention == NormalConvention.OPENGL
                                  else NormalConvention.OPENGL)
        return self

    def adjust_normal_strength(self, strength_factor: float):
        """base.py:689-706: x and y of the normal map times `strength_factor`, renormalised.  The map is replaced by a new tensor
        (upstream also scales the old tensor in place first: INTEGRATION.md, numerical differences)."""
        self.materialize_blend()
        if self._raw.get("normal") is not None:
            f = float(strength_factor)
            self._raw["normal"] = F_.transform_normals(self._resident(keep=True)["normal"], ((f, 0.0), (0.0, f)), True)
        return self

    def compute_normal_from_height(self, scale: float = 1.0):
        """base.py:708-729: the normal map computed from the height map in this material's normal_convention.  A pending lazy blend
        and a pending tile(n, lazy=True) are carried out first: upstream tiles and then differentiates, so the pixels along a seam
        see the neighbouring tile.  A height that requires grad keeps its graph."""
        directx = F_._directx(self.normal_convention)           # argument errors before any device work
        self.materialize_blend()
        if self._raw.get("height") is None:
            raise ValueError("Height map is required to compute normals.")
        height = self._raw["height"]
        if height.dim() == 3 and height.shape[0] != 1:
            raise ValueError("Height map must have 1 channel, got %d" % height.shape[0])
        self.materialize_tile()
        maps = self._resident(keep=True)                        # samples of a PNG become upstream's floats (8 / 16 bit) on the way
        self._raw["normal"] = F_.normal_from_height(maps["height"], scale, "directx" if directx else "opengl")
        self.__dict__["_raw_normal"] = False
        return self

    def compute_height_from_normal(self, scale: float = 1.0):
        """base.py:731-751: the height map reconstructed from the normal map (a Poisson solve, functional.height_from_normal) in this
        material's normal_convention, normalised to [0, 1].  A pending lazy blend and a pending tile(n, lazy=True) are carried out
        first, as for compute_normal_from_height: the solve is periodic over the map it is given.  The result is stored as it comes out
        of the kernel, on the compute device (upstream writes _maps["height"] directly).  A normal map that requires grad keeps its graph."""
        directx = F_._directx(self.normal_convention)           # argument errors before any device work
        self.materialize_blend()
        if self._raw.get("normal") is None:
            raise ValueError("Normal map is required to compute height.")
        self.materialize_tile()
        maps = self._resident(keep=True)                        # a deferred decode of the normal map happens on the way
        self._raw["height"] = F_.height_from_normal(maps["normal"], scale, "directx" if directx else "opengl")
        return self

    # -- the two calls around the BRDF in examples/example_brdf.py:11
    def resize(self, size, antialias: bool = True):
        """Resize every map (base.py:490-504): bilinear, antialiased by default; in place, returns self.  All float32 (C,H,W) maps
        of one size -- a material's maps as a rule -- go through ONE pbr_resize_bilinear launch over all their planes; the results
        stay on the device (module docstring)."""
        self.materialize_tile()
        maps = self._resident(keep=True)
        store = self._raw
        groups = {}
        for name, t in maps.items():
            if t.dim() == 3 and t.dtype == torch.float32 and not (t.requires_grad and torch.is_grad_enabled()):
                groups.setdefault(tuple(t.shape[-2:]), []).append(name)
            else:
                store[name] = F_.resize(t, size, antialias=antialias)
        for names in groups.values():
            names.sort(key=lambda k: maps[k].data_ptr())
            ts = [maps[k] for k in names]
            out = F_.resize(_as_block(ts), size, antialias=antialias)
            p = 0
            for k, t in zip(names, ts):
                store[k] = out[p:p + t.shape[0]]
                p += t.shape[0]
        return self

    # -- pure indexing (base.py:524-537); no arithmetic involved
    def tile(self, num_tiles: int, lazy: bool = False):
        """Repeat every map num_tiles x num_tiles (base.py:524-537).  `lazy=True` (build extension) only records
        the repeat: the maps stay as they are, `CookTorranceBRDF` hands the count to the kernel, which evaluates every texel at
        all its repeats -- each texel then leaves HBM once instead of num_tiles^2 times and no copy is made; whoever else looks at
        the maps sees the repeated ones.  A material whose maps are waiting on the compute device (module docstring), or live there,
        records the repeat likewise."""
        if num_tiles <= 0:                 # upstream: map.repeat(1, 0, 0) -> empty maps; a negative count is torch's RuntimeError
            self.materialize_tile()
            self._samples_on_host()
            store = self._raw
            for name, t in store.items():
                if t is not None:
                    store[name] = t.repeat(*((1,) * (t.dim() - 2) + (num_tiles, num_tiles)))
            return self
        on_device = [t.is_cuda for t in self._raw.values() if t is not None]
        if lazy or self._is_away() or self._has_pending() or (on_device and all(on_device)):
            # maps nobody has seen yet, or maps that live on the compute device: the repeat is recorded and the kernels evaluate (and
            # differentiate) every texel at all its repeats -- the example's `material.resize(512).tile(2)` inside a rendering loss
            # (06_advanced.rst:73-107) then moves a quarter of the map bytes and no repeated copy exists; whoever LOOKS at the maps
            # (`_maps`, attribute access, `as_dict`, `clone`, another map operation) gets the repeated ones, as upstream
            ny, nx = self.lazy_tile
            object.__setattr__(self, "_lazy_tile", (ny * num_tiles, nx * num_tiles))
            return self
        self.materialize_tile()
        store = self._maps
        for name, t in store.items():
            if t is not None:
                reps = (1,) * (t.dim() - 2) + (num_tiles, num_tiles)
                store[name] = t.repeat(*reps)
        return self

    @property
    def lazy_tile(self) -> Tuple[int, int]:
        """Pending (ny, nx) repeat recorded by tile(n, lazy=True); (1, 1) if none."""
        return self.__dict__.get("_lazy_tile", (1, 1))

    def materialize_tile(self):
        """Turns a pending lazy repeat into real maps (anything but the BRDF needs them), where the maps are."""
        ny, nx = self.lazy_tile
        if (ny, nx) != (1, 1):
            object.__setattr__(self, "_lazy_tile", (1, 1))
            self.materialize_blend()
            self._samples_on_host()
            if self.__dict__.get("_raw_normal"):
                self._bring_home_normal()
            store = self._raw
            for name, t in store.items():
                if t is not None:
                    store[name] = t.repeat(*((1,) * (t.dim() - 2) + (ny, nx)))
        return self

    # -- geometric transforms (base.py:506-522, :605-655), in place, returning self; csrc/geometry.hip.  Each is an index map, and so is a
    # chain of them (functional.PlaneMap; transforms.Compose hands a whole run over as `stages`).  As with the normal-map operations above,
    # the normal map is stored as it comes out of the kernel, never through _process_normal_map: a flipped flat normal (0, 0, 1) has no
    # negative value and would be decoded a second time.
    def _geometry(self, stages, fresh: bool = False):
        """Runs geometric stages (functional.fold_stages) over every map.  All float32 (C,H,W) maps of one size go through ONE
        pbr_remap_planes launch per folded map, over all their planes; other maps (batches, fp16) and maps that require grad one at a
        time through the differentiable path.  Everything is checked and folded on the host before any device work.  `fresh`: maps the
        stages leave as they are become copies (the result must not share memory with the maps it was made from)."""
        stages = list(stages)
        ny, nx = self.lazy_tile
        if (ny, nx) != (1, 1):                                   # a recorded tile(n) is the first stage of the chain
            stages.insert(0, ("tile", ny, nx))
        sizes = {tuple(t.shape[-2:]) for t in self._raw.values() if t is not None}
        pending = self.__dict__.get("_lazy_blend")
        if pending is not None:
            sizes |= {tuple(t.shape[-2:]) for t in pending[0].values() if t is not None}
        folded = {hw: F_.fold_stages(hw[0], hw[1], stages) for hw in sizes}      # raises for a crop outside a map
        maps = self._resident(keep=True)
        object.__setattr__(self, "_lazy_tile", (1, 1))
        store = self._raw

        def run(t, chain, negate):
            for pm in chain:
                t = F_.remap_planes(t, pm.ymap, pm.xmap, negate=[p for p, on in zip(negate, pm.neg) if on], out_size=pm.size)
            return t
        groups = {}
        for name, t in maps.items():
            chain = folded[tuple(t.shape[-2:])]
            if not chain:
                store[name] = t.clone() if fresh else t
            elif t.dim() == 3 and t.dtype == torch.float32 and not (t.requires_grad and torch.is_grad_enabled()):
                groups.setdefault(tuple(t.shape[-2:]), []).append(name)
            else:
                c0 = t.dim() - 3
                store[name] = run(t, chain, (0, 1) if name == "normal" and t.shape[c0] >= 2 else ())
        for hw, names in groups.items():
            names.sort(key=lambda k: maps[k].data_ptr())
            while names:                                         # at most 32 planes share a launch (one sign bit per plane)
                take, planes = [], 0
                while names and planes + maps[names[0]].shape[0] <= 32:
                    planes += maps[names[0]].shape[0]
                    take.append(names.pop(0))
                if not take:                                     # a single map of more than 32 planes: plane by plane blocks
                    k = names.pop(0)
                    store[k] = torch.cat([run(maps[k][i:i + 32], folded[hw], ()) for i in range(0, maps[k].shape[0], 32)], dim=0)
                    continue
                ts = [maps[k] for k in take]
                first = {k: sum(t.shape[0] for t in ts[:i]) for i, k in enumerate(take)}
                negate = (first["normal"], first["normal"] + 1) if "normal" in first and maps["normal"].shape[0] >= 2 else ()
                out = run(_as_block(ts), folded[hw], negate)
                for k, t in zip(take, ts):
                    store[k] = out[first[k]:first[k] + t.shape[0]]
        return self

    def crop(self, top: int, left: int, height: int, width: int):
        """base.py:506-522 for crops that lie inside every map; a crop that does not raises ValueError before any device work (upstream
        pads it with zeros through torchvision: INTEGRATION.md)."""
        return self._geometry([("crop", top, left, height, width)])

    def flip_horizontal(self):
        """base.py:605-621: every map mirrored along its width, the normal map's x negated."""
        return self._geometry([("flip_h",)])

    def flip_vertical(self):
        """base.py:623-639: every map mirrored along its height, the normal map's y negated."""
        return self._geometry([("flip_v",)])

    def roll(self, shift: Tuple[int, int]):
        """base.py:641-655: torch.roll over (height, width) by shift = (dy, dx); any integers."""
        dy, dx = shift
        return self._geometry([("roll", int(dy), int(dx))])

    def _shallow(self):
        """A material over the SAME tensors with a map dict of its own (what a fused transforms.Compose run starts from: every map is
        about to be replaced, so nothing is cloned)."""
        new = copy.copy(self)._drop_call_caches()
        new.__dict__["_store"] = dict(self._raw)
        return new

    def clone(self):
        """Deep copy: tensors cloned, flags copied (base.py:880-912)."""
        self.materialize_blend()          # a pending lazy blend is carried out first: the copy must not blend again
        self._samples_on_host()
        if self.__dict__.get("_raw_normal"):
            self._bring_home_normal()
        new = copy.copy(self)._drop_call_caches()
        new.__dict__["_lazy_blend"] = None
        object.__setattr__(new, "_maps", {k: (None if v is None else v.clone()) for k, v in self._raw.items()})
        return new

    @classmethod
    def _assemble(cls, device, maps: dict, **flags):
        """A material of this class around maps this package produced (a conversion): they stay where they were computed."""
        new = cls(device=device, **flags)
        for name, t in maps.items():
            if t is not None:
                new._raw[name] = new._settle(name, t)
        return new

    def __repr__(self):
        body = ", ".join(f"{k}={None if v is None else tuple(v.shape)}" for k, v in self._raw.items())
        return f"{type(self).__name__}({body})"


def _as_block(ts):
    """[P,H,W] over the planes of (C_i,H,W) tensors: a view when they sit back to back in one allocation (functional.upload_packed,
    a previous resize), else a copy."""
    first = ts[0]
    plane = first.shape[-2] * first.shape[-1]
    adjacent = all(t.is_contiguous() for t in ts) and all(
        a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and a.data_ptr() + a.numel() * a.element_size() == b.data_ptr()
        for a, b in zip(ts, ts[1:]))
    if adjacent:
        return first.as_strided((sum(t.shape[0] for t in ts), first.shape[-2], first.shape[-1]), (plane, first.shape[-1], 1))
    return torch.cat(ts, dim=0)


class BasecolorMetallicMaterial(MaterialBase):
    """Metallic workflow (metallic.py:22-69)."""

    def __init__(self, albedo=None, albedo_is_srgb: bool = True, normal=None, roughness=None, metallic=None,
                 **kwargs):
        super().__init__(albedo=albedo, albedo_is_srgb=albedo_is_srgb, normal=normal, roughness=roughness, **kwargs)
        if metallic is not None:
            self.metallic = metallic

    @property
    def basecolor(self):
        return self.albedo

    @basecolor.setter
    def basecolor(self, value):
        self.albedo = value

    def to_diffuse_specular_material(self, albedo_is_srgb: bool = False, specular_is_srgb: bool = True):
        """metallic.py:71-120.  The new material shares normal/roughness, holds LINEAR
        diffuse and specular maps and -- as upstream -- is flagged specular_is_srgb=True
        unless told otherwise."""
        self.materialize_tile()
        self.materialize_blend()
        if self._raw.get("albedo") is None or self._raw.get("metallic") is None:
            raise ValueError("Both albedo and metallic maps are required for conversion.")
        maps = self._resident(keep=True)
        albedo, metallic = maps["albedo"], maps["metallic"]
        if metallic.shape[-2:] != albedo.shape[-2:]:       # metallic.py:93-96: TF.resize(metallic, albedo.shape[1:], antialias=True)
            metallic = F_.resize(metallic, tuple(albedo.shape[-2:]), antialias=True)
        diffuse, specular = F_.metallic_to_diffuse_specular(albedo, metallic, albedo_is_srgb=self.albedo_is_srgb)
        return DiffuseSpecularMaterial._assemble(
            self.device, dict(albedo=diffuse, normal=maps.get("normal"), roughness=maps.get("roughness"), specular=specular),
            albedo_is_srgb=albedo_is_srgb, specular_is_srgb=specular_is_srgb)


class DiffuseSpecularMaterial(MaterialBase):
    """Specular workflow (diffuse.py:23-91)."""

    def __init__(self, albedo=None, albedo_is_srgb: bool = True, normal=None, roughness=None, specular=None,
                 specular_is_srgb: bool = True, **kwargs):
        super().__init__(albedo=albedo, albedo_is_srgb=albedo_is_srgb, normal=normal, roughness=roughness, **kwargs)
        self.specular_is_srgb = specular_is_srgb
        if specular is not None:
            self.specular = specular

    @property
    def diffuse(self):
        return self.albedo

    @diffuse.setter
    def diffuse(self, value):
        self.albedo = value

    @property
    def linear_specular(self):
        """diffuse.py:76-91."""
        specular = self._maps.get("specular")
        if specular is None:
            return None
        return _through_device(specular, F_.srgb_to_linear) if self.specular_is_srgb else specular

    def to_basecolor_metallic_material(self, albedo_is_srgb: bool = False):
        """diffuse.py:93-158: RAW specular (not linear_specular), 3-channel metallic."""
        self.materialize_tile()
        self.materialize_blend()
        if self._raw.get("albedo") is None or self._raw.get("specular") is None:
            raise ValueError("Both albedo (diffuse) and specular maps are required for conversion.")
        maps = self._resident(keep=True)
        albedo, specular = maps["albedo"], maps["specular"]
        if specular.shape[-2:] != albedo.shape[-2:]:       # diffuse.py:117-118: TF.resize(self.specular, diffuse.shape[1:], antialias=True)
            specular = F_.resize(specular, tuple(albedo.shape[-2:]), antialias=True)
        base, metallic = F_.diffuse_specular_to_basecolor_metallic(albedo, specular, albedo_is_srgb=self.albedo_is_srgb)
        return BasecolorMetallicMaterial._assemble(
            self.device, dict(albedo=base, normal=maps.get("normal"), roughness=maps.get("roughness"), metallic=metallic),
            albedo_is_srgb=albedo_is_srgb)

    def to_linear(self):
        """diffuse.py:160-175."""
        super().to_linear()
        if self._raw.get("specular") is not None and self.specular_is_srgb:
            self._convert_in_place("specular", "specular_is_srgb", F_.srgb_to_linear)
            self.specular_is_srgb = False
        return self

    def to_srgb(self):
        """diffuse.py:177-190."""
        super().to_srgb()
        if self._raw.get("specular") is not None and not self.specular_is_srgb:
            self._convert_in_place("specular", "specular_is_srgb", F_.linear_to_srgb)
            self.specular_is_srgb = True
        return self
