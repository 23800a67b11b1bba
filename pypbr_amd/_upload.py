"""Host <-> device movement of maps: results that come home through page-locked memory (`to_host`), maps packed into one device
allocation (`pack_maps`), and a CPU-resident material's upload as ONE transfer (`upload_packed`) with an image's samples turned into
float32 on arrival -- MaterialBase._to_tensor, pypbr/materials/base.py:143-164, and :191-242 behind it for a normal map:
csrc/unpack.hip (pbr_unpack_image).  The way back is its mirror image: float maps become image samples on the device (`pack_image`,
csrc/pack_image.hip, pbr_pack_images: MaterialBase.to_pil, base.py:793-850) and a material's samples come home in ONE transfer
(`download_samples`).  `_staged` is how the family modules run a CPU tensor through the device.

The four settings below are read HERE, so this is the module to assign them on (`from pypbr_amd import _upload as U; U.PLANE_SKEW_BYTES =
4352`); pypbr_amd.functional does not re-export them.  The PBR_* environment variables seed them at import."""
import ctypes
import os
import threading
import weakref
from typing import Optional, Sequence

import torch

from . import _native as N
from ._dispatch import _needs_grad, launch


_PINNED_OUT = []            # weak references to page-locked results still held by callers
PINNED_RESULT_CAP = int(os.environ.get("PBR_PINNED_RESULT_CAP", str(1 << 30)))


def to_host(t: torch.Tensor, device=torch.device("cpu")) -> torch.Tensor:
    """Device -> CPU for results handed back to CPU-resident materials (the reference's default).  `t.cpu()` allocates a
    fresh pageable tensor every time: 26 ms for the 192 MiB result of a 4096^2 material, page faults included.  The
    pinned caching allocator hands back recycled page-locked blocks instead: 3.5 ms, the rate of the link
    (tools/pcie_path_probe.py).  Page-locked memory is a bounded resource and torch never returns such blocks to the OS,
    so at most PINNED_RESULT_CAP bytes (PBR_PINNED_RESULT_CAP, default 1 GiB) of results that callers still hold are
    page-locked; beyond that (a loop that stores its results) the copy is an ordinary pageable one.  Synchronises the
    current stream, as `.cpu()` does.  Plain copy when a gradient is attached (autograd has to see the transfer)."""
    if not t.is_cuda or t.requires_grad:
        return t.to(device)
    nbytes = t.numel() * t.element_size()
    _PINNED_OUT[:] = [r for r in _PINNED_OUT if r() is not None]
    held = sum(r().numel() * r().element_size() for r in _PINNED_OUT if r() is not None)
    if held + nbytes > PINNED_RESULT_CAP:
        return t.to(device)
    try:
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    except RuntimeError:                  # page-locking refused (RLIMIT_MEMLOCK, exhausted pool): the pageable way still works
        return t.to(device)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    _PINNED_OUT.append(weakref.ref(host))
    return host


def _staged(t: torch.Tensor, fn):
    """fn on the device; a CPU tensor travels there and its result back (differentiably when it requires grad)."""
    if t.is_cuda:
        return fn(t)
    N.require_device()
    if _needs_grad(t):
        return fn(t.to("cuda")).to(t.device)
    return to_host(fn(t.to("cuda")), t.device)


def pack_maps(*maps: Optional[torch.Tensor], device=None, reserve_output: bool = False, material_major: bool = False):
    """Copies the maps of a material (or of a batch) into a single device allocation and returns views of it (same
    shapes, dtypes and values; `None` stays `None`).  Pure data movement (torch copies), no arithmetic.  Why: a launch
    streams all planes of a material at once, and planes that live in one allocation sit close together in the
    address space; `reserve_output=True` also appends room for the fp32 result and returns it last, so that `out=`
    can be placed next to its inputs.  `material_major=True` (batched [B,C,H,W] maps): material b's planes and its
    result next to each other, materials one pitch apart -- strided views, which the C ABI takes as they are.  It
    is an option, not the default: measured 3-4 % ahead for 16 x 4096^2, level for 64 x 2048^2, 2-5 % behind for
    64 x 1024^2 (tools/batch_layout_probe.py).  See DESIGN.md, "Data layout in HBM", for the measurements."""
    present = [t for t in maps if t is not None]
    if not present:
        return tuple(maps) + ((None,) if reserve_output else ())
    dev = torch.device(device) if device is not None else present[0].device

    def padded(nbytes):                                  # every map starts 256-byte aligned
        return -(-nbytes // 256) * 256
    batch = max([t.shape[0] for t in present if t.dim() == 4] or [1])
    if batch > 1 and material_major:
        return _pack_material_major(maps, batch, dev, reserve_output, padded)
    out_shape = None
    if reserve_output:
        out_shape = tuple(present[0].shape[:-3]) + (3,) + tuple(present[0].shape[-2:])

    def pitch_of(shape, esz):
        """Bytes from one plane of a map to the next.  Planes whose size is a multiple of 8 MiB (2048^2, 4096^2 fp32 ...)
        all start on the same HBM channel group when packed back to back; PLANE_SKEW_BYTES (when set) more per plane
        spread them (tools/skew_probe.py: 16 x 2048^2 with every tensor skewed, linear order: 6.16 -> 6.44 TB/s; inside
        one arena the effect is ~1 %, see below).  Other sizes stay dense."""
        plane = shape[-2] * shape[-1] * esz
        return plane + (PLANE_SKEW_BYTES if PLANE_SKEW_BYTES and plane % (8 << 20) == 0 else 0)

    def extent(shape, esz):
        n_planes = 1
        for d in shape[:-2]:
            n_planes *= d
        return padded(n_planes * pitch_of(shape, esz))
    sizes = [0 if t is None else extent(t.shape, t.element_size()) for t in maps]
    out_bytes = extent(out_shape, 4) if reserve_output else 0
    arena = _aligned_arena(sum(sizes) + out_bytes, dev)

    def view(off, shape, dtype, esz):
        pitch = pitch_of(shape, esz) // esz
        strides = [1, shape[-1]]
        step = pitch
        for d in reversed(shape[:-2]):
            strides.append(step)
            step *= d
        strides = tuple(reversed(strides))            # (..., planes, rows, 1): dense rows, `pitch` elements between planes
        typed = arena.view(dtype)
        return typed.as_strided(tuple(shape), strides, typed.storage_offset() + off // esz)
    views, off = [], 0
    for t, nbytes in zip(maps, sizes):
        if t is None:
            views.append(None)
            continue
        v = view(off, t.shape, t.dtype, t.element_size())
        v.copy_(t)
        views.append(v)
        off += nbytes
    if reserve_output:
        views.append(view(off, out_shape, torch.float32, 4))
    return tuple(views)


# The page-locked staging area of upload_packed, one per thread, reused: allocating one is a hipHostMalloc (4 ms for 10 MB) and torch's
# caching host allocator handed a recycled block back only some of the time -- the upload of examples/example_brdf.py's material took 0.8
# or 4.5 ms by that alone (tools/example_bench.py, per-repeat times).  Grown geometrically; requests beyond the cap get a block of their own.
UPLOAD_STAGE_CAP = int(os.environ.get("PBR_UPLOAD_STAGE_CAP", str(256 << 20)))
_UPLOAD_STAGE = threading.local()


def _upload_stage(nbytes: int):
    """-> (`nbytes` of page-locked uint8 -- pageable where page-locking is refused: still one transfer --, the slot to leave the copy's
    event in or None).  The previous copy out of the slot is waited for before its memory is handed out again."""
    def fresh(n):
        try:
            return torch.empty(n, dtype=torch.uint8, pin_memory=True)
        except RuntimeError:
            return torch.empty(n, dtype=torch.uint8)
    if nbytes > UPLOAD_STAGE_CAP:
        return fresh(nbytes), None
    slot = getattr(_UPLOAD_STAGE, "slot", None)
    if slot is None or slot[0].numel() < nbytes:
        grown = max(nbytes, 2 * slot[0].numel() if slot is not None else 0)
        slot = _UPLOAD_STAGE.slot = [fresh(min(grown, UPLOAD_STAGE_CAP)), None]
    if slot[1] is not None:
        slot[1].synchronize()
        slot[1] = None
    return slot[0][:nbytes], slot


def release_upload_stage():
    """Drops the CALLING thread's page-locked staging block (up to UPLOAD_STAGE_CAP bytes stay pinned per uploading thread otherwise:
    loader pools and server threads that are done uploading call this, or set PBR_UPLOAD_STAGE_CAP lower).  The copy still in flight
    out of it is waited for first."""
    slot = getattr(_UPLOAD_STAGE, "slot", None)
    if slot is not None:
        if slot[1] is not None:
            slot[1].synchronize()
        _UPLOAD_STAGE.slot = None


# Host tensor -> its place in the staging area.  Up to this many bytes per upload the copy is a plain memcpy on the calling thread, NOT
# Tensor.copy_: ATen spreads a host copy over its whole OpenMP pool (128 threads on a GPU box's 256-core host), whose workers then spin
# on every core -- inside the box's CPU quota (16 cores) that stalled this very thread for 70-170 ms at a time (CFS throttling: every other
# upload of examples/example_brdf.py's 10 MB of samples), and each munmap that followed paid TLB shootdowns to all of them (2-5 ms to free
# the samples).  Measured with tools/upload_phase_probe.py: 0.4-0.6 ms, every time, for the same bytes by memcpy.  Above the limit (a
# 4096^2 float material is 537 MB) the pool's bandwidth is worth more than that risk.
STAGE_MEMCPY_LIMIT = int(os.environ.get("PBR_STAGE_MEMCPY_LIMIT", str(128 << 20)))


def _page_locked_range(samples):
    """Dense sample arrays that all live in ONE page-locked storage, each dword-aligned, covering a range not much larger than their
    bytes -> (address of the range's first byte, its length, the range as a uint8 tensor); None otherwise."""
    first = samples[0]
    storage = first.untyped_storage()
    if not all(t.untyped_storage().data_ptr() == storage.data_ptr() for t in samples) or not first.is_pinned():
        return None
    lo = min(t.data_ptr() for t in samples)
    hi = max(t.data_ptr() + t.numel() * t.element_size() for t in samples)
    used = sum(t.numel() * t.element_size() for t in samples)
    if any((t.data_ptr() - lo) % 4 for t in samples) or lo % 4 or hi - lo > 2 * used + 4096:
        return None
    whole = torch.empty(0, dtype=torch.uint8).set_(storage)
    start = lo - storage.data_ptr()
    return lo, hi - lo, whole[start:start + (hi - lo)]


def _stage_copy(dst_bytes: torch.Tensor, src: torch.Tensor, upload_bytes: int):
    # a host memcpy: only a HOST source may take it (a device pointer here would be read by the CPU, unordered against the kernels
    # still queued on that device); anything else goes through copy_, which knows about devices and streams
    if upload_bytes <= STAGE_MEMCPY_LIMIT and src.device.type == "cpu" and src.is_contiguous():
        ctypes.memmove(dst_bytes.data_ptr(), src.data_ptr(), dst_bytes.numel())
    else:
        dst_bytes.view(src.dtype).view(src.shape).copy_(src)


ENCODED_DTYPES = (torch.uint8, torch.uint16)       # an image's own samples (materials._image_to_tensor(..., defer=True)); float32 / 255 or / 65535 once decoded


def is_encoded(t) -> bool:
    return t is not None and t.dtype in ENCODED_DTYPES


def _dense_samples(t: torch.Tensor):
    """(C,H,W) view of image samples -> (the dense array behind it, (stride_c, stride_h, stride_w) in samples).  PIL's (H,W,C) array
    seen as (C,H,W) travels as it is; anything that is not one dense block is copied to (C,H,W) order first."""
    C, H, W = t.shape
    hwc = t.permute(1, 2, 0)
    if hwc.is_contiguous():
        return hwc, (1, W * C, C)
    t = t.contiguous()
    return t, (H * W, W, 1)


def unpack_image(samples: torch.Tensor, bits: int, strides, shape, out: torch.Tensor, decode_normal: bool = False) -> torch.Tensor:
    """MaterialBase._to_tensor for PIL images (base.py:143-164) on the device: `bits`-wide samples (8 | 16) starting at `samples`'
    first byte, resident on `out`'s device, addressed [c*strides[0] + y*strides[1] + x*strides[2]] -> float32 (C,H,W) `out` (dense);
    with `decode_normal` base.py:191-242 follows in the same pass and `out` is (3,H,W) (pbr_unpack_image)."""
    C, H, W = shape
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != ((3 if decode_normal else C), H, W) or samples.device != out.device:
        raise ValueError("unpack_image: `out` must be a contiguous float32 (C,H,W) tensor on the samples' device")
    launch(out.device, N.lib().pbr_unpack_image, samples.data_ptr(), bits, C, H, W, strides[0], strides[1], strides[2],
           out.data_ptr(), 1 if decode_normal else 0)
    return out


_SAMPLE_DTYPES = {8: torch.uint8, 16: torch.uint16}


def _image_pack(t: torch.Tensor, dst_ptr: int, bits: int, encode_normal: bool) -> N.ImagePack:
    """One row of a pbr_pack_images table: the (C,H,W) float32 device tensor `t`, read through its own strides."""
    return N.ImagePack(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2), dst_ptr, t.shape[0], bits, 1 if encode_normal else 0, 0)


def _pack_images_call(device, rows, height: int, width: int) -> None:
    """One call into pbr_pack_images: at most N.MAX_IMAGE_PACKS maps of one (height, width), one launch."""
    table = (N.ImagePack * len(rows))(*rows)
    launch(device, N.lib().pbr_pack_images, table, len(rows), height, width)


def _float_map(t: torch.Tensor, what: str) -> torch.Tensor:
    """The (C,H,W) float32 map the kernel reads.  A float16 map is converted to float32 FIRST: its samples are those of the float32
    values (upstream would multiply in half precision and round the product to half before truncating)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError("%s takes a (C,H,W) map, got %s" % (what, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
    if t.dtype == torch.float16:
        t = t.float()
    if t.dtype != torch.float32:
        raise TypeError("%s supports float32 (float16 is converted to float32 first), got %s" % (what, t.dtype))
    if not 1 <= t.shape[0] <= 4:
        raise ValueError("%s: a map has 1 to 4 channels, got %d" % (what, t.shape[0]))
    if min(t.shape) < 1:
        raise ValueError("%s: empty map %s" % (what, tuple(t.shape)))
    return t.detach()


def pack_image(t: torch.Tensor, bits: int = 8, encode_normal: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaterialBase.to_pil's arithmetic for ONE map (base.py:793-850) on the device: float32 (C,H,W) `t`, any strides -> the (H,W,C)
    sample tensor on `t`'s device, uint8 (`bits` 8: torchvision's pic.mul(255).byte()) or uint16 (`bits` 16: base.py:837), a normal
    map through (n + 1.0) * 0.5 first (`encode_normal`, 3 channels).  Inside [0, 1] upstream's samples bit for bit; outside it the
    samples saturate and NaN gives 0 (include/pbr_hip.h, pbr_pack_images).  float32 only: a float16 map is converted to float32 first.
    `out`: a contiguous (H,W,C) tensor of the sample type on `t`'s device.  A CPU tensor travels to the device and its samples back."""
    if bits not in _SAMPLE_DTYPES:
        raise TypeError("pack_image: bits must be 8 or 16, got %r" % (bits,))
    t = _float_map(t, "pack_image")
    C, H, W = t.shape
    if encode_normal and C != 3:
        raise ValueError("pack_image: a normal map has 3 channels, got %d" % C)
    if not t.is_cuda:
        if out is not None:
            raise ValueError("pack_image: `out` goes with a map on a ROCm device")
        return _staged(t, lambda d: pack_image(d, bits, encode_normal))
    if out is None:
        out = torch.empty((H, W, C), dtype=_SAMPLE_DTYPES[bits], device=t.device)
    elif out.dtype != _SAMPLE_DTYPES[bits] or tuple(out.shape) != (H, W, C) or not out.is_contiguous() or out.device != t.device:
        raise ValueError("pack_image: `out` must be a contiguous (H,W,C) %s tensor on the map's device" % _SAMPLE_DTYPES[bits])
    _pack_images_call(t.device, [_image_pack(t, out.data_ptr(), bits, encode_normal)], H, W)
    return out


def download_samples(maps: dict, bits, normal_name: str = "normal") -> dict:
    """name -> float (C,H,W) map on ONE ROCm device  ->  name -> numpy (H,W,C) samples on the host, uint8 or uint16 as `bits` says (an
    int for all maps, or a dict name -> 8 | 16, 8 where it has no entry); the map called `normal_name` is encoded as a normal map.  The
    samples of all maps are written into one device arena, each map 256-byte aligned, by ONE pbr_pack_images call per (H, W) group
    (per N.MAX_IMAGE_PACKS maps of it), and come home in ONE device-to-host copy through `to_host` (page-locked, subject to
    PINNED_RESULT_CAP).  The arrays are views of that one block: no per-map copy, no arithmetic on the host."""
    names = [k for k, t in maps.items() if t is not None]
    if not names:
        return {}
    ts = {k: _float_map(maps[k], "download_samples") for k in names}
    dev = ts[names[0]].device
    if dev.type != "cuda" or any(t.device != dev for t in ts.values()):
        raise RuntimeError("download_samples needs every map on one ROCm device; there is no CPU path")
    width = {k: (bits.get(k, 8) if isinstance(bits, dict) else bits) for k in names}
    if any(b not in _SAMPLE_DTYPES for b in width.values()):
        raise TypeError("download_samples: bits must be 8 or 16, got %r" % (bits,))
    if normal_name in ts and ts[normal_name].shape[0] != 3:
        raise ValueError("download_samples: a normal map has 3 channels, got %d" % ts[normal_name].shape[0])
    offs, total = {}, 0
    for k in names:
        offs[k] = total
        total += -(-ts[k].numel() * (width[k] // 8) // 256) * 256
    arena = _aligned_arena(total, dev)
    groups = {}
    for k in names:
        groups.setdefault(tuple(ts[k].shape[-2:]), []).append(k)
    for (H, W), members in groups.items():
        for i in range(0, len(members), N.MAX_IMAGE_PACKS):
            rows = [_image_pack(ts[k], arena.data_ptr() + offs[k], width[k], k == normal_name) for k in members[i:i + N.MAX_IMAGE_PACKS]]
            _pack_images_call(dev, rows, H, W)
    host = to_host(arena).numpy()
    out = {}
    for k in names:
        C, H, W = ts[k].shape
        n = C * H * W * (width[k] // 8)
        out[k] = host[offs[k]:offs[k] + n].view("uint8" if width[k] == 8 else "uint16").reshape(H, W, C)
    return out


def upload_packed(tensors: Sequence[torch.Tensor], device, tail_planes: int = 0, encoded_normal: Optional[int] = None):
    """CPU tensors -> tensors on `device` with ONE host-to-device copy: the maps are laid out in a page-locked host arena exactly as
    they will sit in the device allocation, which then arrives as a single DMA transfer (five separate `t.to(device)` of pageable
    tensors are five transfers, each bounced through the runtime's own staging buffers).  Maps that share dtype and (H, W) -- a
    material's maps as a rule -- are packed as DENSE planes, so that the whole material is one [P,H,W] block: whole-material
    operations (MaterialBase.resize) then take one launch over all planes; `tail_planes` more planes of that shape are left free
    behind them (a float normal map's decoded form lands there).  Otherwise every map starts 256-byte aligned.

    Maps that are still an image's samples (uint8 / uint16, `is_encoded`) travel AS SAMPLES -- a quarter / half of the bytes -- in a
    staging area in front of the block and are turned into float32 on arrival (pbr_unpack_image, one launch per map; the map at index
    `encoded_normal` is a normal map and is decoded on the way, base.py:191-242); their float planes sit behind the planes of the
    maps that arrived as floats, so that the copy stays ONE contiguous transfer and the block stays dense.

    Returns (views in the order given, the [P + tail_planes, H, W] block or None)."""
    dev = torch.device(device)
    ts = [t.detach() for t in tensors]
    if not ts:
        return [], None
    enc = [is_encoded(t) for t in ts]
    out_dtype = [torch.float32 if e else t.dtype for t, e in zip(ts, enc)]
    out_shape = [((3,) + tuple(t.shape[1:]) if i == encoded_normal else tuple(t.shape)) for i, t in enumerate(ts)]
    same = all(d == out_dtype[0] and t.dim() == 3 and t.shape[-2:] == ts[0].shape[-2:] for t, d in zip(ts, out_dtype))

    def slot_bytes(i):
        n = out_dtype[i].itemsize
        for e in out_shape[i]:
            n *= e
        return n if same else -(-n // 256) * 256

    # staging area (samples), then the maps that arrive as floats, then the unpacked maps, then the tail
    dense, stage_off, off = {}, {}, 0
    for i, t in enumerate(ts):
        if enc[i]:
            dense[i] = _dense_samples(t)
            stage_off[i] = off
            off += -(-dense[i][0].numel() * t.element_size() // 256) * 256
    # Samples the loader decoded straight into ONE page-locked block (io.load_material_from_folder) are already where a DMA transfer can
    # read them, laid out for it: the block's used range goes up as it is -- no staging copy, and nothing to free but the block itself.
    direct = _page_locked_range([dense[i][0] for i in range(len(ts))]) if all(enc) and dev.type == "cuda" else None
    if direct is not None:
        base, off = direct[0], -(-direct[1] // 256) * 256
        stage_off = {i: dense[i][0].data_ptr() - base for i in range(len(ts))}
    staged = off
    offs = {}
    for i in [i for i in range(len(ts)) if not enc[i]] + [i for i in range(len(ts)) if enc[i]]:
        offs[i] = off
        off += slot_bytes(i)
    sent = staged + sum(slot_bytes(i) for i in range(len(ts)) if not enc[i])           # bytes of the one transfer
    plane = ts[0].shape[-2] * ts[0].shape[-1] * out_dtype[0].itemsize
    total = off + (tail_planes * plane if same else 0)
    if direct is not None:
        host, stage = direct[2], None
    else:
        host, stage = _upload_stage(sent)
        for i, t in enumerate(ts):
            src, o = (dense[i][0], stage_off[i]) if enc[i] else (t, offs[i])
            _stage_copy(host[o:o + src.numel() * src.element_size()], src, sent)
    arena = _aligned_arena(total, dev)
    arena[:host.numel()].copy_(host, non_blocking=True)
    if stage is not None and dev.type == "cuda":
        stage[1] = torch.cuda.Event()
        stage[1].record(torch.cuda.current_stream(dev))
    views = []
    for i, t in enumerate(ts):
        n = out_dtype[i].itemsize
        for e in out_shape[i]:
            n *= e
        view = arena[offs[i]:offs[i] + n].view(out_dtype[i]).view(out_shape[i])
        if enc[i]:
            unpack_image(arena[stage_off[i]:], 8 * t.element_size(), dense[i][1], tuple(t.shape), view, decode_normal=(i == encoded_normal))
        views.append(view)
    block = None
    if same:
        block = arena[staged:].view(out_dtype[0]).view(-1, ts[0].shape[-2], ts[0].shape[-1])
    return views, block


# 0 = dense planes (the default).  Measured with 4352 (17 x 256 B, tools/skew_ab.sh): batches of 2048^2 maps +1 %
# (16 maps: 467.6 -> 462.5 us), 64 x 2048^2 +0.6 %, 4 x 4096^2 level, the bench workload (one 4096^2 material) 1.5 % SLOWER
# (114.0 -> 116.1 us) -- so it stays an experiment knob.
PLANE_SKEW_BYTES = int(os.environ.get("PBR_PLANE_SKEW_BYTES", "0"))


def _aligned_arena(nbytes, dev):
    """`nbytes` of uint8 whose first byte is 256-byte aligned IN MEMORY, whatever the allocator hands out (the device
    allocator already aligns to 512; the host allocator only to 64)."""
    raw = torch.empty(nbytes + 255, dtype=torch.uint8, device=dev)
    skip = -raw.data_ptr() % 256
    return raw[skip:skip + nbytes]


def _pack_material_major(maps, batch, dev, reserve_output, padded):
    """Batched maps [B,C,H,W]: material b's planes (and its result) next to each other, materials one pitch apart.
    The views keep their [B,C,H,W] shapes; only the batch stride differs from a free-standing tensor, which the C ABI
    takes per map.  Maps shared by the whole batch ([1,C,H,W]) are stored once, behind the materials."""
    per_material = [t for t in maps if t is not None and t.dim() == 4 and t.shape[0] == batch]
    if any(t is not None and not (t.dim() == 4 and t.shape[0] in (1, batch)) for t in maps):
        raise ValueError("batched maps must all be [B,C,H,W] or [1,C,H,W]")
    h, w = per_material[0].shape[-2:]
    pitch = sum(padded(t[0].numel() * t.element_size()) for t in per_material)
    out_bytes = padded(3 * h * w * 4) if reserve_output else 0
    pitch += out_bytes
    shared_bytes = sum(padded(t.numel() * t.element_size()) for t in maps if t is not None and t.shape[0] == 1)
    arena = _aligned_arena(batch * pitch + shared_bytes, dev)
    views, off, shared_off = [], 0, batch * pitch
    for t in maps:
        if t is None:
            views.append(None)
            continue
        es, plane = t.element_size(), t.shape[-2] * t.shape[-1]
        typed = arena.view(t.dtype)
        if t.shape[0] == 1:
            v = typed.as_strided(tuple(t.shape), (t[0].numel(), plane, t.shape[-1], 1), typed.storage_offset() + shared_off // es)
            shared_off += padded(t.numel() * es)
        else:
            v = typed.as_strided(tuple(t.shape), (pitch // es, plane, t.shape[-1], 1), typed.storage_offset() + off // es)
            off += padded(t[0].numel() * es)
        v.copy_(t)
        views.append(v)
    if reserve_output:
        typed = arena.view(torch.float32)
        views.append(typed.as_strided((batch, 3, h, w), (pitch // 4, h * w, w, 1), typed.storage_offset() + off // 4))
    return tuple(views)
