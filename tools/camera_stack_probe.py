#!/usr/bin/env python3
"""The light-stack steps under the perspective camera on one S x S metallic material, point lights, the candidates alternating in one process:
  (a) rendering_loss_mse_stack(view_type="point").backward() with the maps requiring grad -- the fused route, one
      pbr_cook_torrance_camera_mse_stack_step;
  (b) the same with maps, lights and intensities requiring grad -- one pbr_cook_torrance_camera_mse_stack_fit_step;
  (c) the composition the same two calls took before the steps existed: L differentiable camera renders, torch.stack, mse_loss, L
      pbr_cook_torrance_camera_backward launches and autograd's accumulation of L gradient sets;
  (d) the orthographic stack step and fit step of the same build on the same maps (view_type="directional"): the same bytes, so what the
      camera costs.
HIP events around forward + backward, 3 warm-ups, the median of 20.  STACK_LAUNCHES must show that (a) and (b) took the fused route.

    python tools/camera_stack_probe.py [--out profiles/camera_stack_probe.json] [--size 4096] [--lights 1,2,8,16] [--maps f32,f16] [--append]

`--append` merges the records into an existing file (same stamp), so that a job can give every (maps, L) step a process and a time limit of
its own."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_material  # noqa: E402
from pypbr_amd import _native as N, functional as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_stack_probe.json"))
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--lights", default="1,2,8,16")
ap.add_argument("--maps", default="f32,f16")
ap.add_argument("--append", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
REPS, WARM = 20, 3
S = args.size
DTYPES = {"f32": torch.float32, "f16": torch.float16}


def median_us(fns):
    """Median time of each callable, the callables alternating inside every repetition."""
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
    return [statistics.median(t) for t in times]


records = []
for tag in args.maps.split(","):
    dtype = DTYPES[tag]
    maps = synth_material(S, dev, 3, dtype)
    for L in [int(v) for v in args.lights.split(",")]:
        ang = torch.arange(L, dtype=torch.float32) * (2 * math.pi / max(L, 3))
        lights0 = torch.stack([0.4 * torch.cos(ang), 0.4 * torch.sin(ang), torch.full((L,), 1.0)], 1)
        common = dict(light_type="point", light_size=1.0)
        camera = dict(common, view_dir=[0.1, -0.2, 1.5], view_type="point")
        ortho = dict(common, view_dir=[0.0, 0.0, 1.0])
        with torch.no_grad():
            targets = F.cook_torrance_stack(*synth_material(S, dev, 4, dtype), light=lights0 * 1.1, light_intensity=torch.ones(L, 3), **camera)
        lights = lights0.to(dev).requires_grad_(True)
        intens = torch.ones(L, 3, device=dev, requires_grad=True)
        leaves = [t.clone().requires_grad_(True) for t in maps]

        def run(kw, fused, fit):
            lt, it = (lights, intens) if fit else (lights.detach(), intens.detach())

            def fn():
                for t in leaves + [lights, intens]:
                    t.grad = None
                if fused:
                    loss = F.rendering_loss_mse_stack(*leaves, targets=targets, light=lt, light_intensity=it, **kw)
                else:       # cook_torrance_stack under a gradient is L differentiable one-light renders: what the call was before the steps
                    loss = TF.mse_loss(F.cook_torrance_stack(*leaves, light=lt, light_intensity=it, **kw), targets)
                loss.backward()
            return fn

        before = dict(F.STACK_LAUNCHES)
        t = median_us([run(camera, True, False), run(camera, True, True), run(camera, False, False), run(camera, False, True),
                       run(ortho, True, False), run(ortho, True, True)])
        n = WARM + REPS
        took = {k: F.STACK_LAUNCHES[k] - before[k] for k in before}
        assert took["camera_mse_stack_step"] == n and took["camera_mse_stack_fit_step"] == n, took      # (a) and (b) took the fused route
        assert took["mse_stack_step"] == n and took["mse_stack_fit_step"] == n and took["camera_stack"] == 0, took
        rec = {"size": S, "maps": tag, "lights": L,
               "a_camera_step_us": round(t[0], 1), "b_camera_fit_step_us": round(t[1], 1),
               "c_composition_maps_us": round(t[2], 1), "c_composition_maps_and_lights_us": round(t[3], 1),
               "d_orthographic_step_us": round(t[4], 1), "d_orthographic_fit_step_us": round(t[5], 1),
               "a_over_c": round(t[0] / t[2], 4), "b_over_c": round(t[1] / t[3], 4), "a_over_d": round(t[0] / t[4], 4), "b_over_d": round(t[1] / t[5], 4)}
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del targets, leaves, lights, intens
        torch.cuda.empty_cache()
    del maps
    torch.cuda.empty_cache()

stamp = N.build_stamp()
out = {"what": "light stacks under the perspective camera (csrc/ct_camera_stack.hip): the fused step and fit step against the composition "
               "(L camera renders, torch.stack, mse_loss, L camera backwards) and against the orthographic stack steps of the same build; "
               "one %d^2 metallic material, point lights (tools/camera_stack_probe.py)" % S,
       "timing": "HIP events around forward + backward of the Python call, %d warm-ups, median of %d, the candidates alternating in one process" % (WARM, REPS),
       "size": S, "device": torch.cuda.get_device_name(0), "stamp": stamp, "records": records}
if args.append and os.path.exists(args.out):
    old = json.load(open(args.out))
    assert old["stamp"] == stamp and old["size"] == S, "the file holds another build's or another size's records"
    out["records"] = old["records"] + records
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
