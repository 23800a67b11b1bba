#!/usr/bin/env python3
"""The stack-fit step on one 4096^2 and one 1024^2 material, fp32 and fp16 maps, point lights, L = 1, 2, 4, 8, 16, the candidates alternating in
one process:
  (a) rendering_loss_mse_stack(...).backward() with maps, lights and intensities requiring grad -- the fused route, one
      pbr_cook_torrance_mse_stack_fit_step -- against the composition that call took before the step existed: L differentiable one-light
      cook_torrance calls, torch.stack, mse_loss, L pbr_cook_torrance_backward_params launches and autograd's accumulation;
  (b) the same two with only lights and intensities requiring grad;
  (c) the bare pbr_cook_torrance_mse_stack_fit_step call against the bare pbr_cook_torrance_mse_stack_step call: the price of the light gradients.
HIP events, 3 warm-ups, the median of 20.  Writes a stamped JSON file.
python tools/light_stack_fit_probe.py [--out profiles/light_stack_fit_step.json] [--sizes 4096,1024] [--lights 1,2,4,8,16]"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_material  # noqa: E402
from pypbr_amd import _native as N, functional as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "light_stack_fit_step.json"))
ap.add_argument("--sizes", default="4096,1024")
ap.add_argument("--lights", default="1,2,4,8,16")
args = ap.parse_args()
dev = torch.device("cuda", 0)
REPS, WARM = 20, 3


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
for S in [int(s) for s in args.sizes.split(",")]:
    for dtype, tag in ((torch.float32, "f32"), (torch.float16, "f16")):
        maps = synth_material(S, dev, 3, dtype)
        for L in [int(v) for v in args.lights.split(",")]:
            ang = torch.arange(L, dtype=torch.float32) * (2 * math.pi / max(L, 3))
            lights0 = torch.stack([0.4 * torch.cos(ang), 0.4 * torch.sin(ang), torch.full((L,), 1.0)], 1)
            kw = dict(view_dir=[0.0, 0.0, 1.0], light_type="point", light_size=1.0)
            with torch.no_grad():
                targets = F.cook_torrance_stack(*synth_material(S, dev, 4, dtype), light=lights0 * 1.1, light_intensity=torch.ones(L, 3), **kw)
            lights = lights0.to(dev).requires_grad_(True)
            intens = torch.ones(L, 3, device=dev, requires_grad=True)
            leaves = [t.clone().requires_grad_(True) for t in maps]

            def run(fused, with_maps):
                ms = leaves if with_maps else maps

                def fn():
                    for t in leaves + [lights, intens]:
                        t.grad = None
                    if fused:
                        loss = F.rendering_loss_mse_stack(*ms, targets=targets, light=lights, light_intensity=intens, **kw)
                    else:       # what the call was before the fit step: cook_torrance_stack under a gradient is L differentiable one-light calls
                        loss = TF.mse_loss(F.cook_torrance_stack(*ms, light=lights, light_intensity=intens, **kw), targets)
                    loss.backward()
                return fn

            plan = F.plan_cook_torrance(*maps, light=lights0, light_intensity=torch.ones(L, 3), **kw)
            grads = [torch.empty_like(t) for t in maps]
            loss, gp = torch.empty((), device=dev), torch.empty(3 + 6 * L, device=dev)
            lib, stream = N.lib(), torch.cuda.current_stream(dev).cuda_stream
            ws = torch.empty(lib.pbr_mse_stack_fit_workspace_bytes(ctypes.byref(plan.desc)) // 8, dtype=torch.float64, device=dev)

            def fit_call():
                N.check(lib.pbr_cook_torrance_mse_stack_fit_step(ctypes.byref(plan.desc), targets.data_ptr(), *[g.data_ptr() for g in grads], None,
                                                                 gp.data_ptr(), loss.data_ptr(), ws.data_ptr(), stream))

            def step_call():
                N.check(lib.pbr_cook_torrance_mse_stack_step(ctypes.byref(plan.desc), targets.data_ptr(), *[g.data_ptr() for g in grads], None,
                                                             loss.data_ptr(), ws.data_ptr(), stream))

            before = F.STACK_LAUNCHES["mse_stack_fit_step"]
            t = median_us([run(True, True), run(False, True), run(True, False), run(False, False), fit_call, step_call])
            assert F.STACK_LAUNCHES["mse_stack_fit_step"] == before + 2 * (WARM + REPS)        # the fused candidates took the fused route
            rec = {"size": S, "maps": tag, "lights": L,
                   "a_fused_maps_and_lights_us": t[0], "a_composition_maps_and_lights_us": t[1], "a_speedup": t[1] / t[0],
                   "b_fused_lights_only_us": t[2], "b_composition_lights_only_us": t[3], "b_speedup": t[3] / t[2],
                   "c_fit_step_call_us": t[4], "c_stack_step_call_us": t[5], "c_ratio": t[4] / t[5]}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del targets, leaves, grads, plan, ws
        del maps
        torch.cuda.empty_cache()

out = {"what": "light stack with light gradients: the fused stack-fit step against the composition (L one-light calls with parameter gradients), "
               "and the bare fit call against the bare stack step (tools/light_stack_fit_probe.py)",
       "timing": "HIP events, %d warm-ups, median of %d, the candidates alternating in one process" % (WARM, REPS),
       "device": torch.cuda.get_device_name(0), "stamp": N.build_stamp(), "records": records}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
