"""`MaterialAdam`: the optimiser step of a fit -- Adam and the projection every map needs behind it, for all maps of a material in ONE
launch (csrc/adam.hip, pbr_adam_step; an extension: upstream has no optimiser).

    groups = material_param_groups(material, lr=1e-2)             # albedo, metallic, specular in [0, 1]; roughness above a floor;
    opt = MaterialAdam(groups)                                    # the normal a unit vector on the camera's side
    loss = MultiLightRenderingLoss(...)(material, photographs); loss.backward(); opt.step()

In exact arithmetic the update is torch.optim.Adam's (weight_decay 0, no amsgrad, no maximize); tools/adam_oracle.py states the order of
operations.  What differs: that order, the rule that an element whose update is exactly 0 keeps its bits -- the part of the
initial maps no photograph covers stays untouched, neither clamped nor renormalised -- and float16 parameters, which carry a float32 `master`
copy in the state.  The state has torch's names and shapes (`step`, `exp_avg`, `exp_avg_sq`), so a state dict travels to torch.optim.Adam
and back.  There is no CPU path: step() needs parameters on a ROCm device.
"""
import math

import torch

from . import _native as N
from ._dispatch import _DTYPES, launch, plane_geometry, rows_are_dense

# Launches since import, by entry point (what the tests count; never reset here).
LAUNCHES = {"adam_step": 0, "adam_advance": 0}

_INF = float("inf")


def _check_group(group):
    """The ValueErrors of construction, per group."""
    if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
        raise ValueError("MaterialAdam has no weight_decay, amsgrad or maximize")
    lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
    if not isinstance(lr, torch.Tensor) and lr < 0:
        raise ValueError("Invalid learning rate: %s" % (lr,))
    if isinstance(lr, torch.Tensor) and not group.get("capturable", False):
        raise ValueError("lr as a tensor needs capturable=True")
    if not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0:
        raise ValueError("Invalid betas: %s" % ((b1, b2),))
    if eps < 0:
        raise ValueError("Invalid epsilon value: %s" % (eps,))
    project, bounds = group.get("project"), group.get("bounds")
    if project not in (None, "unit"):
        raise ValueError("project is None or 'unit', got %r" % (project,))
    if project == "unit":
        if bounds is not None:
            raise ValueError("a 'unit' group takes min_z, not bounds")
        for p in group["params"]:
            if p.dim() not in (3, 4) or p.shape[-3] != 3:
                raise ValueError("'unit' projects [3,H,W] / [B,3,H,W] tensors, got shape %s" % (tuple(p.shape),))
    elif group.get("min_z") is not None:
        raise ValueError("min_z belongs to a 'unit' group")
    if bounds is not None:
        if len(bounds) != 2:
            raise ValueError("bounds is (lo, hi); either may be None")
        lo, hi = bounds
        if lo is not None and hi is not None and lo > hi:
            raise ValueError("bounds: lo %s > hi %s" % (lo, hi))


def _coefficients(lr, betas, eps, t):
    """pbr_adam_coeffs of one group at step count t: float64, rounded once (tools/adam_oracle.py: coefficients)."""
    b1, b2 = float(betas[0]), float(betas[1])
    return N.AdamCoeffs(float(lr) / (1.0 - b1 ** float(t)), 1.0 / math.sqrt(1.0 - b2 ** float(t)), 1.0 - b1, b2, 1.0 - b2, float(eps))


def _planes(t):
    """(tensor, batch, channels, pixels, batch stride, plane stride) with dense planes, or None: [C,H,W] / [B,C,H,W] views of packed maps
    keep their strides; anything else counts as one plane of numel elements when it is contiguous."""
    if t.dim() in (3, 4):
        if not rows_are_dense(t):
            return None
        batch, channels, h, w, batch_stride, plane_stride = plane_geometry(t)
        return t, batch, channels, h * w, batch_stride, plane_stride
    if t.is_contiguous():
        return t, 1, 1, t.numel(), 0, 0
    return None


class MaterialAdam(torch.optim.Optimizer):
    """MaterialAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, capturable=False).  Group options: `lr`, `betas`, `eps`, and the
    projection applied to the parameter behind every step -- `bounds=(lo, hi)` (clamp; either may be None), or `project="unit"` with an
    optional `min_z` for [3,H,W] / [B,3,H,W] normals (z <- max(z, min_z), then F.normalize over the channels).  float32 and float16
    parameters; gradients in the parameter's dtype; `exp_avg` and `exp_avg_sq` always float32, and float16 parameters keep a float32 `master`
    in the state that the update runs on.  step() gathers every parameter that has a gradient into tables of at most
    N.MAX_ADAM_TENSORS and launches pbr_adam_step once per table, on the current stream, without synchronising.
    `capturable=True`: `step` is a device tensor, the coefficients are formed on the device (pbr_adam_advance, one small launch in front of
    every table), `lr` may be a 0-dim float32 device tensor, and zero_grad / loss / backward / step capture into one torch.cuda.graph."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, capturable=False, **unsupported):
        for name in ("weight_decay", "amsgrad", "maximize"):
            if unsupported.pop(name, 0):
                raise ValueError("MaterialAdam has no %s" % name)
        if unsupported:
            raise TypeError("MaterialAdam: unexpected arguments %s" % sorted(unsupported))
        # (the keys torch.optim.Adam reads from a group, at the values this optimiser implements: a state dict loads there)
        defaults = dict(lr=lr, betas=betas, eps=eps, project=None, bounds=None, min_z=None, capturable=bool(capturable), weight_decay=0, amsgrad=False,
                        maximize=False, foreach=None, differentiable=False, fused=None, decoupled_weight_decay=False)
        self._coeffs = {}                     # capturable: the device coefficient table of every launch, by its position
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        """torch's, behind the ValueErrors of construction (a refused group is not added)."""
        probe = dict(self.defaults)
        probe.update(param_group)
        params = probe["params"]
        probe["params"] = [params] if isinstance(params, torch.Tensor) else list(params)
        _check_group(probe)
        param_group = dict(param_group)
        param_group["params"] = probe["params"]
        super().add_param_group(param_group)

    def load_state_dict(self, state_dict):
        """torch's, and then: options a foreign state dict (torch.optim.Adam's) does not carry keep this optimiser's values, and the float32
        state of float16 parameters is float32 again (torch casts loaded state to the parameter's dtype)."""
        mine = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, before in zip(self.param_groups, mine):
            for k, v in before.items():
                group.setdefault(k, v)
            _check_group(group)
        saved = state_dict["state"]
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, params):
            if i in saved and p.dtype == torch.float16:
                for k in ("exp_avg", "exp_avg_sq", "master"):
                    if k in saved[i]:
                        self.state[p][k] = saved[i][k].detach().to(device=p.device, dtype=torch.float32).clone()

    def _state_of(self, p, capturable):
        state = self.state[p]
        if "step" not in state:
            state["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if capturable else torch.tensor(0.0, dtype=torch.float32)
        if "exp_avg" not in state:
            state["exp_avg"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            state["exp_avg_sq"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        if p.dtype == torch.float16 and "master" not in state:
            state["master"] = p.detach().to(torch.float32).contiguous()
        return state

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries = []                         # (param, entry, group, state)
        for group in self.param_groups:
            lo, hi = group["bounds"] if group.get("bounds") is not None else (None, None)
            if group.get("project") == "unit":
                kind = N.ADAM_UNIT
            else:
                kind = N.ADAM_BOX if group.get("bounds") is not None else N.ADAM_NONE
            min_z = group.get("min_z")
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("MaterialAdam.step needs parameters on a ROCm device; there is no CPU path")
                if p.dtype not in _DTYPES:
                    raise TypeError("MaterialAdam supports float32/float16 parameters, got %s" % p.dtype)
                if p.grad.is_sparse:
                    raise RuntimeError("MaterialAdam does not support sparse gradients")
                geom = _planes(p)
                if geom is None:
                    raise ValueError("MaterialAdam needs parameters with dense planes (a [C,H,W] / [B,C,H,W] view of packed maps, or contiguous)")
                g = p.grad if p.grad.dtype == p.dtype else p.grad.to(p.dtype)
                ggeom = _planes(g)
                if ggeom is None:                          # a gradient that is not plane-dense (an expanded one, a transposed one)
                    g = g.contiguous()
                    ggeom = _planes(g)
                state = self._state_of(p, group["capturable"])
                for k in ("exp_avg", "exp_avg_sq", "master"):
                    if k in state and not (state[k].is_contiguous() and state[k].dtype == torch.float32 and state[k].device == p.device):
                        state[k] = state[k].to(device=p.device, dtype=torch.float32).contiguous()
                _, batch, channels, pixels, p_bs, p_ps = geom
                master = state["master"].data_ptr() if p.dtype == torch.float16 else None
                e = N.AdamTensor(p.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), master, pixels,
                                 p_bs, p_ps, ggeom[4], ggeom[5], batch, channels, _DTYPES[p.dtype], kind,
                                 -_INF if lo is None else float(lo), _INF if hi is None else float(hi), -_INF if min_z is None else float(min_z), 0)
                entries.append((p, e, group, state, g))
        for first in range(0, len(entries), N.MAX_ADAM_TENSORS):
            self._launch(first // N.MAX_ADAM_TENSORS, entries[first:first + N.MAX_ADAM_TENSORS])
        for p, *_ in entries:
            torch.autograd.graph.increment_version(p)      # the kernel wrote through a raw pointer: autograd and the caches must see an edit
        return loss

    def _launch(self, index, chunk):
        n = len(chunk)
        device = chunk[0][0].device
        if any(p.device != device for p, *_ in chunk):
            raise RuntimeError("MaterialAdam: the parameters of one step live on one device")
        table = (N.AdamTensor * n)(*[e for _, e, _, _, _ in chunk])
        capturable = chunk[0][2]["capturable"]
        if any(group["capturable"] != capturable for _, _, group, _, _ in chunk):
            raise ValueError("MaterialAdam: capturable is one choice for all groups")
        if capturable:
            # one coefficient row per parameter: every parameter has its own device counter (torch's capturable `step`)
            rows = (N.AdamGroup * n)()
            for i, (p, _, group, state, _) in enumerate(chunk):
                step, lr = state["step"], group["lr"]
                if not (isinstance(step, torch.Tensor) and step.is_cuda and step.dtype == torch.float32):
                    state["step"] = step = torch.as_tensor(float(step), dtype=torch.float32).to(device)
                lr_ptr = None
                if isinstance(lr, torch.Tensor):
                    if not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1):
                        raise ValueError("a tensor lr is one float32 value on the parameters' device")
                    lr_ptr = lr.data_ptr()
                rows[i] = N.AdamGroup(step.data_ptr(), lr_ptr, 0.0 if lr_ptr else float(lr), float(group["betas"][0]), float(group["betas"][1]),
                                      float(group["eps"]))
                table[i].group = i
            coeffs = self._coeffs.get((index, device))
            if coeffs is None:
                coeffs = self._coeffs[(index, device)] = torch.zeros(N.MAX_ADAM_TENSORS, 6, dtype=torch.float32, device=device)
            launch(device, N.lib().pbr_adam_advance, rows, n, coeffs.data_ptr())
            LAUNCHES["adam_advance"] += 1
            launch(device, N.lib().pbr_adam_step, table, n, None, coeffs.data_ptr(), n)
        else:
            slots, host = {}, []
            for i, (p, _, group, state, _) in enumerate(chunk):
                step = state["step"]
                t = float(step) + 1.0
                if isinstance(step, torch.Tensor):
                    step += 1
                else:
                    state["step"] = t
                key = (id(group), t)
                if key not in slots:
                    slots[key] = len(host)
                    host.append(_coefficients(group["lr"], group["betas"], group["eps"], t))
                table[i].group = slots[key]
            launch(device, N.lib().pbr_adam_step, table, n, (N.AdamCoeffs * len(host))(*host), None, len(host))
        LAUNCHES["adam_step"] += 1


_BOUNDED = ("albedo", "metallic", "specular")


def material_param_groups(material, lr=1e-3, lr_normal=None, roughness_min=0.05, min_z=0.0, maps=None):
    """The parameter groups of a material's stored maps for MaterialAdam: albedo, metallic and specular with bounds=(0, 1), roughness with
    bounds=(roughness_min, 1) -- below about 0.1 the GGX denominator cancels; 0.05 is the lower end of the criterion inputs -- the normal
    with project="unit" and `min_z` (at `lr_normal`, default `lr`), height without a projection.  `maps`: the names to fit (default: every
    stored map of those six).  Sets requires_grad_ on the maps it returns; the maps are the material's own tensors, updated in place."""
    names = list(material._fit_maps()) if maps is None else list(maps)
    groups = []
    for name, t in zip(names, material._stored(names)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError("the material has no decoded %r map to fit" % name)
        t.requires_grad_(True)
        if name == "normal":
            groups.append({"params": [t], "lr": lr if lr_normal is None else lr_normal, "project": "unit", "min_z": min_z})
        elif name == "roughness":
            groups.append({"params": [t], "lr": lr, "bounds": (roughness_min, 1.0)})
        elif name in _BOUNDED:
            groups.append({"params": [t], "lr": lr, "bounds": (0.0, 1.0)})
        else:
            groups.append({"params": [t], "lr": lr})
    return groups
