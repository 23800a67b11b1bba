"""The host-side caches' shared parts: the settings, "are these still the very same tensors", the host snapshot of a light / view
parameter, the tensor-keyed memo and the kept plan.  Pure Python over torch -- neither `functional` nor `_native` is imported here -- so
what counts as "unchanged" is decided in one place and is testable without a device."""
import os
import threading
import weakref
from typing import Optional

import torch

# ------------------------------------------------------------------ caches keyed on tensor identity + version counter
# Three caches save repeated work on tensors that did not change between calls: the device copy of a CPU-resident material
# (models.CookTorranceBRDF), the host copy of device-resident light / view tensors (functional._host_vec3) and the "already signed?"
# verdict of a normal map (materials).  They recognise "did not change" by object identity and `tensor._version` -- which is NOT
# bumped by `t.data.add_()`, by edits of a numpy array that shares the tensor's memory (`torch.from_numpy(a).float()` shares
# it for float32 arrays, and materials ingest arrays exactly so, as upstream does), or by kernels that write through raw
# pointers (`out=`).  The reference re-reads its maps and parameters on every call, so all three are OFF by default and
# opt-in: `set_caching(device_maps=True, parameters=True, decode_verdicts=True)`, or PBR_CACHE=maps,params,decode in the
# environment, for loops that are known not to edit their tensors behind autograd's back.  Inference tensors
# (torch.inference_mode) have no version counter at all and are never cached.
CACHING = {"device_maps": False, "parameters": False, "decode_verdicts": False}
for _tok, _key in (("maps", "device_maps"), ("params", "parameters"), ("decode", "decode_verdicts")):
    if _tok in os.environ.get("PBR_CACHE", "").split(","):
        CACHING[_key] = True


def set_caching(device_maps: Optional[bool] = None, parameters: Optional[bool] = None, decode_verdicts: Optional[bool] = None) -> dict:
    """Switches the identity + version keyed caches (see above) on or off; returns the previous settings."""
    old = dict(CACHING)
    for key, v in (("device_maps", device_maps), ("parameters", parameters), ("decode_verdicts", decode_verdicts)):
        if v is not None:
            CACHING[key] = bool(v)
    return old


def version_of(t: torch.Tensor):
    """`t._version`, or None for tensors that do not track one (created under torch.inference_mode): those are not cached."""
    try:
        return None if t.is_inference() else t._version
    except RuntimeError:
        return None


def weak_refs(tensors):
    return tuple(None if t is None else weakref.ref(t) for t in tensors)


def same_tensors(refs, tensors) -> bool:
    """Are `tensors` still the very objects `refs` (weak_refs) were taken of?  None matches None only."""
    return len(refs) == len(tensors) and all((r is None and t is None) or (r is not None and r() is t) for r, t in zip(refs, tensors))


def host_values(v):
    """Snapshot of a host-resident view / light / intensity, to tell at the next call whether its VALUES changed; None for anything
    a kept plan cannot follow (tensors on the device or with a gradient, other types)."""
    if isinstance(v, torch.Tensor):
        return None if v.is_cuda or v.requires_grad else v.tolist()
    if isinstance(v, (list, tuple)):                          # a copy: the caller may edit its list in place between calls
        return [list(r) if isinstance(r, (list, tuple)) else r for r in v]
    return None


class VersionMemo:
    """id(tensor) -> (weakref to it, its version, payload): a hit needs the same object (an id is reused once its tensor is freed) at the
    same version.  Small: dead entries are swept on every `put`, and at `limit` entries everything is forgotten."""

    def __init__(self, limit: int = 64):
        self.limit, self._entries = limit, {}

    def get(self, t, version):
        e = self._entries.get(id(t))
        return e[2] if e is not None and e[0]() is t and e[1] == version else None

    def put(self, t, version, payload):
        for k in [k for k, e in self._entries.items() if e[0]() is None]:
            del self._entries[k]
        if len(self._entries) >= self.limit:
            self._entries.clear()
        self._entries[id(t)] = (weakref.ref(t), version, payload)

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()


class ValueMemo:
    """key (hashable host values) -> payload, for host-side plans that depend on nothing but their arguments (functional.rotate_plan: the
    constants of one rotation).  Nothing to invalidate; at `limit` entries everything is forgotten."""

    def __init__(self, limit: int = 256):
        self.limit, self._entries = limit, {}

    def get(self, key, make):
        """The payload of `key`, made by `make()` on a miss (an exception from `make` is the caller's and caches nothing)."""
        hit = self._entries.get(key)
        if hit is None:
            hit = make()
            if len(self._entries) >= self.limit:
                self._entries.clear()
            self._entries[key] = hit
        return hit

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()


class KeptPlan:
    """A functional.RenderPlan kept between calls: pointers, never values of maps.  `maps` are held weakly, `values` are the host_values the
    descriptor was last filled from, `lock` serialises refill + launch through this one descriptor (taken non-blocking: a busy entry is
    bypassed, not waited for), `out_shape` is the result to allocate per call (None: the loss step writes no colour)."""
    __slots__ = ("plan", "maps", "values", "lock", "out_shape")

    def __init__(self, plan, maps, values, out_shape=None):
        self.plan, self.maps, self.values, self.out_shape = plan, weak_refs(maps), values, out_shape
        self.lock = threading.Lock()

    @classmethod
    def adopt(cls, plan, maps, values, out_shape=None):
        """The entry for `plan` built from `maps` (in the plan's order: albedo, normal, roughness, metallic, specular), or None.  Only a plan
        that points INTO the caller's own tensors (no staging copy, no device parameter block) is kept: their owner keeps them alive for as
        long as it wants the plan, so the plan lets go of them -- a resize() / to() / assignment that replaces the store frees the old maps
        at once instead of leaving e.g. 537 MB of 4K maps pinned behind a descriptor nobody will launch again."""
        if plan._param_block is not None or not all(p is None or (t is not None and p.data_ptr() == t.data_ptr()) for p, t in zip(plan._keep, maps)):
            return None
        plan._keep = ()
        return cls(plan, maps, values, out_shape)

    def describes(self, maps) -> bool:
        return same_tensors(self.maps, maps)

    def try_acquire(self) -> bool:
        return self.lock.acquire(False)

    def release(self):
        self.lock.release()

    def refresh(self, values) -> bool:
        """Parameter values are re-read every call: the descriptor is refilled when they changed.  False: they describe another number of
        lights -- another kernel, so the caller builds another plan."""
        if values != self.values:
            if not self.plan.refill(*values):
                return False
            self.values = values
        return True
