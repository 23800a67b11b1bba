#!/usr/bin/env python3
"""Light stacks with one camera position per shot (csrc/ct_view_stack.hip) on one S x S metallic material, point lights, the candidates
alternating in one process:
  (a) rendering_loss_mse_stack(view_type="point", view_dir=[L,3]).backward() with the maps requiring grad -- the fused route, one
      pbr_cook_torrance_view_mse_stack_step;
  (b) the same with maps, cameras, lights and intensities requiring grad -- one pbr_cook_torrance_view_mse_stack_fit_step;
  (i) what the same fit cost before [L,3] positions existed: L single-shot rendering_loss_mse(view_type="point", view_dir=C_l, light=light_l,
      target=targets[l]) calls averaged, then one backward -- through the package at `--parent DIR` (a build of the parent commit, imported
      under an alias like tools/ab_revisions.py does) when given, else through this build's own single-shot path;
  (ii) the fixed-camera stack step and fit step of this build on the same maps and L (one position for all shots): the same bytes, so the
      price of the per-shot view.
HIP events around forward + backward, 3 warm-ups, the median of 20; `spread` is the largest (max - min) / median over the candidates' 20
samples.  STACK_LAUNCHES must show that (a) and (b) took the fused route.

    python tools/view_stack_probe.py [--out profiles/view_stack_probe.json] [--size 4096] [--lights 1,2,8,16] [--maps f32,f16] [--parent DIR]

Without `--one` the tool opens no device itself: it gives every (maps, L) step a child process and a time limit of its own (`--limit`
seconds), the children append their record to the file, and nothing is started after a child that failed or ran out of time."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_stack_probe.json"))
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


def load_parent(path):
    """The parent build's package under an alias: its own host code, its own libpbr_hip.so (tools/ab_revisions.py: load_revision)."""
    import importlib.util
    pkg_dir = os.path.join(os.path.abspath(path), "pypbr_amd")
    name = "pypbr_rev_parent"
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".functional"), importlib.import_module(name + "._native")


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
        kw = dict(light_type="point", light_size=1.0, view_type="point")
        with torch.no_grad():
            targets = F.cook_torrance_stack(*synth_material(S, dev, 4, dtype), view_dir=cams0 * 1.05, light=lights0 * 1.1, light_intensity=torch.ones(L, 3), **kw)
        cams = cams0.to(dev).requires_grad_(True)
        lights = lights0.to(dev).requires_grad_(True)
        intens = torch.ones(L, 3, device=dev, requires_grad=True)
        fixed = cams0.mean(dim=0).to(dev).requires_grad_(True)
        leaves = [t.clone().requires_grad_(True) for t in maps]
        params = [cams, lights, intens, fixed]

        def stack(view, fit):
            def fn():
                for t in leaves + params:
                    t.grad = None
                v, lt, it = (view, lights, intens) if fit else (view.detach(), lights.detach(), intens.detach())
                F.rendering_loss_mse_stack(*leaves, targets=targets, view_dir=v, light=lt, light_intensity=it, **kw).backward()
            return fn

        def shots(fit):
            def fn():
                for t in leaves + params:
                    t.grad = None
                v, lt, it = (cams, lights, intens) if fit else (cams.detach(), lights.detach(), intens.detach())
                total = None
                for l in range(L):
                    one = PF.rendering_loss_mse(*leaves, target=targets[l], view_dir=v[l], light=lt[l], light_intensity=it[l], **kw)
                    total = one if total is None else total + one
                (total / L).backward()
            return fn

        before = dict(F.STACK_LAUNCHES)
        t, spread = measure([stack(cams, False), stack(cams, True), shots(False), shots(True), stack(fixed, False), stack(fixed, True)])
        n = WARM + REPS
        took = {k: F.STACK_LAUNCHES[k] - before[k] for k in before}
        if L > 1:                                           # (at L = 1, [1,3] is one position for all shots: the fixed-camera steps serve it)
            assert took["view_mse_stack_step"] == n and took["view_mse_stack_fit_step"] == n, took          # (a) and (b) took the fused route
        rec = {"size": S, "maps": tag, "lights": L,
               "a_view_step_us": round(t[0], 1), "b_view_fit_step_us": round(t[1], 1),
               "i_single_shots_maps_us": round(t[2], 1), "i_single_shots_all_us": round(t[3], 1),
               "ii_fixed_camera_step_us": round(t[4], 1), "ii_fixed_camera_fit_step_us": round(t[5], 1),
               "a_over_i": round(t[0] / t[2], 4), "b_over_i": round(t[1] / t[3], 4), "a_over_ii": round(t[0] / t[4], 4), "b_over_ii": round(t[1] / t[5], 4),
               "spread": round(max(spread), 4), "single_shots_from": "parent build" if args.parent else "this build"}
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del targets, leaves, cams, lights, intens, fixed, params
        torch.cuda.empty_cache()
    del maps
    torch.cuda.empty_cache()

stamp = N.build_stamp()
out = {"what": "light stacks with one camera position per shot (csrc/ct_view_stack.hip): the fused step and fit step against L single-shot "
               "rendering_loss_mse(view_type='point') calls averaged and one backward, and against the fixed-camera stack steps of the same "
               "build; one %d^2 metallic material, point lights (tools/view_stack_probe.py)" % S,
       "timing": "HIP events around forward + backward of the Python call, %d warm-ups, median of %d, the candidates alternating in one process, "
                 "one process per record; spread = the largest (max - min) / median over a record's candidates" % (WARM, REPS),
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
