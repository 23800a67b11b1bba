#!/usr/bin/env python3
"""The light-stack loss steps with per-pixel weights (csrc/ct_stack_weighted.hip, ct_camera_stack_weighted.hip, ct_view_stack_weighted.hip) on
one S x S metallic material, point lights, one weight plane per shot, the candidates alternating in one process.  Per family -- orthographic
view, one camera position, one camera position per shot:
  (a) rendering_loss_mse_stack(weights=).backward() with the maps requiring grad -- one weighted step;
  (b) the same with maps, view / cameras, lights and intensities requiring grad -- one weighted fit step;
  (i) what the same weighted loss costs without the weighted steps, which is the composition: cook_torrance_stack with gradients (L renders,
      torch.stack), (w * (stack - targets) ** 2).mean(), L backwards -- for maps alone and for maps and parameters; through the package at
      `--parent DIR` (a build of the parent commit, imported under an alias like tools/ab_revisions.py does) when given, else through this
      build's own composition;
  (ii) the UNWEIGHTED step and fit step of this build on the same maps: 64 + 12 L bytes per pixel against 64 + 16 L.
HIP events around forward + backward, 3 warm-ups, the median of 20; `spread` is the largest (max - min) / median over a family's candidates'
20 samples.  STACK_LAUNCHES must show that (a), (b) and (ii) took the fused routes.

    python tools/weighted_stack_probe.py [--out profiles/weighted_stack_probe.json] [--size 4096] [--lights 1,2,8,16] [--maps f32,f16] [--parent DIR]

Without `--one` the tool opens no device itself: it gives every (maps, L) step a child process and a time limit of its own (`--limit`
seconds), the children append their records to the file, and nothing is started after a child that failed or ran out of time."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_stack_probe.json"))
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--lights", default="1,2,8,16")
ap.add_argument("--maps", default="f32,f16")
ap.add_argument("--parent", default=None, help="a tree with a build of the parent commit: (i) runs through its package")
ap.add_argument("--limit", type=int, default=150, help="seconds a (maps, L) step may take")
ap.add_argument("--one", action="store_true", help="measure here (one process): what the driver starts per step")
args = ap.parse_args()

if not args.one:
    if os.path.exists(args.out):
        os.remove(args.out)
    for tag in args.maps.split(","):
        for L in args.lights.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", "--out", args.out, "--size", str(args.size), "--lights", L, "--maps", tag]
            if args.parent:
                cmd += ["--parent", args.parent]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                sys.exit("step maps=%s L=%s ended with status %d: nothing more is started" % (tag, L, rc))
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
from bench import synth_material  # noqa: E402
from pypbr_amd import _native as N, functional as F  # noqa: E402

dev = torch.device("cuda", 0)
REPS, WARM = 20, 3
S = args.size
DTYPES = {"f32": torch.float32, "f16": torch.float16}
FAMILIES = (("orthographic", "directional", "mse_stack"), ("camera", "point", "camera_mse_stack"), ("view", "point", "view_mse_stack"))


def load_parent(path):
    """The parent build's package under an alias: its own host code, its own libpbr_hip.so (tools/ab_revisions.py: load_revision)."""
    import importlib.util
    pkg_dir = os.path.join(os.path.abspath(path), "pypbr_amd")
    name = "pypbr_rev_parent"
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    PF, PN = importlib.import_module(name + ".functional"), importlib.import_module(name + "._native")
    if hasattr(PF, "USE_TORCH_OPS"):
        PF.USE_TORCH_OPS = False                          # the registered operators exist once per process: the parent through its ctypes plans
    return PF, PN


PF, PN = load_parent(args.parent) if args.parent else (F, N)


def measure(fns):
    """(median, (max - min) / median) of each callable's time in us, the callables alternating inside every repetition."""
    times = [[] for _ in fns]
    for rep in range(WARM + REPS):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= WARM:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return [statistics.median(t) for t in times], [(max(t) - min(t)) / statistics.median(t) for t in times]


records = []
for tag in args.maps.split(","):
    dtype = DTYPES[tag]
    maps = synth_material(S, dev, 3, dtype)
    for L in [int(v) for v in args.lights.split(",")]:
        ang = torch.arange(L, dtype=torch.float32) * (2 * math.pi / max(L, 3))
        lights0 = torch.stack([0.4 * torch.cos(ang), 0.4 * torch.sin(ang), torch.full((L,), 1.0)], 1)
        cams0 = lights0 * torch.tensor([0.9, 0.9, 1.0]) + torch.tensor([0.02, -0.03, 0.5])      # the lens a few centimetres from the flash, further out
        g = torch.Generator().manual_seed(7 + L)
        weights = torch.rand(L, 1, S, S, generator=g) * 2.0                                      # a plane per shot, a quarter of it masked out
        weights[torch.rand(L, 1, S, S, generator=g) < 0.25] = 0.0
        weights = weights.to(dev)
        for family, view_type, counter in FAMILIES:
            view0 = {"orthographic": torch.tensor([0.05, 0.1, 0.9]), "camera": cams0.mean(dim=0), "view": cams0}[family]
            if family == "view" and L == 1:
                continue                                     # [1,3] is one position for all shots: the camera family's row
            kw = dict(light_type="point", light_size=1.0, view_type=view_type)
            with torch.no_grad():
                targets = F.cook_torrance_stack(*synth_material(S, dev, 4, dtype), view_dir=view0 * 1.05, light=lights0 * 1.1,
                                                light_intensity=torch.ones(L, 3), **kw)
            view = view0.to(dev).requires_grad_(True)
            lights = lights0.to(dev).requires_grad_(True)
            intens = torch.ones(L, 3, device=dev, requires_grad=True)
            leaves = [t.clone().requires_grad_(True) for t in maps]
            params = [view, lights, intens]

            def parameters(fit):
                return (view, lights, intens) if fit else (view.detach(), lights.detach(), intens.detach())

            def fused(fit, w):
                def fn():
                    for t in leaves + params:
                        t.grad = None
                    v, lt, it = parameters(fit)
                    extra = {} if w is None else {"weights": w}
                    F.rendering_loss_mse_stack(*leaves, targets=targets, view_dir=v, light=lt, light_intensity=it, **extra, **kw).backward()
                return fn

            def composed(fit):
                def fn():
                    for t in leaves + params:
                        t.grad = None
                    v, lt, it = parameters(fit)
                    stack = PF.cook_torrance_stack(*leaves, view_dir=v, light=lt, light_intensity=it, **kw)
                    (weights * (stack - targets) ** 2).mean().backward()
                return fn

            before = dict(F.STACK_LAUNCHES)
            t, spread = measure([fused(False, weights), fused(True, weights), composed(False), composed(True), fused(False, None), fused(True, None)])
            n = WARM + REPS
            took = {k: F.STACK_LAUNCHES[k] - before[k] for k in before}
            weighted = counter.replace("mse_stack", "weighted_mse_stack")
            assert took[weighted + "_step"] == n and took[weighted + "_fit_step"] == n, took          # (a) and (b) took the weighted routes
            assert took[counter + "_step"] == n and took[counter + "_fit_step"] == n, took            # (ii) the unweighted ones
            rec = {"size": S, "maps": tag, "lights": L, "family": family,
                   "a_weighted_step_us": round(t[0], 1), "b_weighted_fit_step_us": round(t[1], 1),
                   "i_composition_maps_us": round(t[2], 1), "i_composition_all_us": round(t[3], 1),
                   "ii_unweighted_step_us": round(t[4], 1), "ii_unweighted_fit_step_us": round(t[5], 1),
                   "a_over_i": round(t[0] / t[2], 4), "b_over_i": round(t[1] / t[3], 4), "a_over_ii": round(t[0] / t[4], 4), "b_over_ii": round(t[1] / t[5], 4),
                   "bytes_ratio": round((64 + 16 * L) / (64 + 12 * L), 4),
                   "spread": round(max(spread), 4), "spread_fused": round(max(spread[:2] + spread[4:]), 4),
                   "composition_from": "parent build" if args.parent else "this build"}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del targets, leaves, view, lights, intens, params
            torch.cuda.empty_cache()
        del weights
        torch.cuda.empty_cache()
    del maps
    torch.cuda.empty_cache()

stamp = N.build_stamp()
out = {"what": "the light-stack loss steps with per-pixel weights, one plane per shot: the weighted step and fit step of the three families "
               "against the composition (cook_torrance_stack with gradients, the weighted mean, L backwards) and against the unweighted steps of "
               "the same build; one %d^2 metallic material, point lights (tools/weighted_stack_probe.py)" % S,
       "timing": "HIP events around forward + backward of the Python call, %d warm-ups, median of %d, the candidates alternating in one process, "
                 "one process per (maps, L); spread = the largest (max - min) / median over a record's candidates, spread_fused over its "
                 "four one-pass candidates" % (WARM, REPS),
       "size": S, "device": torch.cuda.get_device_name(0), "stamp": stamp, "records": records}
if args.parent:
    out["parent_stamp"] = PN.build_stamp()
if os.path.exists(args.out):
    old = json.load(open(args.out))
    assert old["stamp"] == stamp and old["size"] == S, "the file holds another build's or another size's records"
    out["records"] = old["records"] + records
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
