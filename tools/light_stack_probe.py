#!/usr/bin/env python3
"""Light stacks on one 4096^2 and one 1024^2 material, fp32 and fp16 maps, point light, L = 1, 2, 4, 8, 16: the fused step
(rendering_loss_mse_stack -> pbr_cook_torrance_mse_stack_step, and that call alone through the C ABI) against L steps of rendering_loss_mse with
autograd's accumulation, alternating in one process; and the forward stack (one pbr_cook_torrance_stack launch) against L cook_torrance
launches.  HIP events, 3 warm-ups, the median of 20; algorithmic bytes from the shapes.  Writes a stamped JSON file.
python tools/light_stack_probe.py [--out profiles/light_stack_step.json] [--sizes 4096,1024] [--lights 1,2,4,8,16]"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_material  # noqa: E402
from pypbr_amd import _native as N, functional as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "light_stack_step.json"))
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
    for dtype, tag, esz in ((torch.float32, "f32", 4), (torch.float16, "f16", 2)):
        maps = synth_material(S, dev, 3, dtype)
        for L in [int(v) for v in args.lights.split(",")]:
            ang = torch.arange(L, dtype=torch.float32) * (2 * math.pi / max(L, 3))
            lights = torch.stack([0.4 * torch.cos(ang), 0.4 * torch.sin(ang), torch.full((L,), 1.0)], 1)
            intens = torch.ones(L, 3)
            kw = dict(view_dir=[0.0, 0.0, 1.0], light_type="point", light_size=1.0)
            with torch.no_grad():
                targets = F.cook_torrance_stack(*synth_material(S, dev, 4, dtype), light=lights, light_intensity=intens, **kw)
            leaves = [t.clone().requires_grad_(True) for t in maps]

            def fused():
                for t in leaves:
                    t.grad = None
                F.rendering_loss_mse_stack(*leaves, targets=targets, light=lights, light_intensity=intens, **kw).backward()

            def steps():
                for t in leaves:
                    t.grad = None
                for l in range(L):
                    (F.rendering_loss_mse(*leaves, target=targets[l], light=lights[l], light_intensity=intens[l], **kw) / L).backward()

            plan = F.plan_cook_torrance(*maps, light=lights, light_intensity=intens, **kw)
            grads = [torch.empty_like(t) for t in maps]
            loss = torch.empty((), device=dev)
            lib, stream = N.lib(), torch.cuda.current_stream(dev).cuda_stream
            ws = torch.empty(max(1, lib.pbr_mse_step_workspace_bytes(ctypes.byref(plan.desc)) // 4), device=dev)

            def fused_call():
                N.check(lib.pbr_cook_torrance_mse_stack_step(ctypes.byref(plan.desc), targets.data_ptr(), *[g.data_ptr() for g in grads], None,
                                                             loss.data_ptr(), ws.data_ptr(), stream))

            def stack_forward():
                with torch.no_grad():
                    F.cook_torrance_stack(*maps, light=lights, light_intensity=intens, **kw)

            def forward_launches():
                with torch.no_grad():
                    for l in range(L):
                        F.cook_torrance(*maps, light=lights[l], light_intensity=intens[l], **kw)

            t_fused, t_steps, t_call, t_stack, t_launches = median_us([fused, steps, fused_call, stack_forward, forward_launches])
            px = S * S
            step_bytes = (16 * esz + 12 * L) * px                         # 8 map planes in, 8 gradient planes out, L targets in
            steps_bytes = ((16 * esz + 12) * L + 24 * esz * (L - 1)) * px   # L one-light steps + autograd's accumulation (read, read, write)
            fwd_bytes = (8 * esz + 12 * L) * px
            rec = {"size": S, "maps": tag, "lights": L,
                   "fused_step_autograd_us": t_fused, "l_steps_autograd_us": t_steps, "speedup": t_steps / t_fused,
                   "fused_step_call_us": t_call, "fused_step_bytes": step_bytes, "fused_step_call_TBps": step_bytes / t_call / 1e6,
                   "l_steps_bytes": steps_bytes,
                   "stack_forward_us": t_stack, "l_forward_launches_us": t_launches, "stack_forward_bytes": fwd_bytes,
                   "stack_forward_TBps": fwd_bytes / t_stack / 1e6}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del targets, leaves, grads, plan
        del maps
        torch.cuda.empty_cache()

out = {"what": "light stack: fused step against L one-light steps with autograd's accumulation; forward stack against L launches (tools/light_stack_probe.py)",
       "timing": "HIP events, %d warm-ups, median of %d, the candidates alternating in one process" % (WARM, REPS),
       "device": torch.cuda.get_device_name(0), "stamp": N.build_stamp(), "records": records}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
