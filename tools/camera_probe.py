#!/usr/bin/env python3
"""The perspective camera against the orthographic kernels of the same shape: one S x S metallic material, one point light, fp32 and fp16
maps, the candidates alternating in one process --
  forward            pbr_cook_torrance_camera            against pbr_cook_torrance
  backward           pbr_cook_torrance_camera_backward   against pbr_cook_torrance_backward            (gradients of the maps)
  backward + params  the same with g_params               against pbr_cook_torrance_backward_params    (camera | view, light, intensity)
The bytes per pixel are the same on both sides (fp32 forward: 32 in, 12 out), so the orthographic time on the same box is the yardstick.
HIP events around single launches, 3 warm-ups, the median of 20.  Writes a stamped JSON file.

    python tools/camera_probe.py [--out profiles/camera_probe.json] [--size 4096]
    python tools/camera_probe.py --counters pmc_run      # merges a `rocprofv3 --pmc SQ_INSTS_VALU` run of `--launch-only` into the file
    rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d pmc_run -o run -- python tools/camera_probe.py --launch-only

`--launch-only`: every candidate twice, untimed -- the run the counters are collected in (a run of its own: counters serialise the kernels).
VALU instructions per pixel = SQ_INSTS_VALU (wave instructions) x 64 lanes / pixels: what one lane issues for one pixel."""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_material  # noqa: E402
from pypbr_amd import _native as N, functional as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_probe.json"))
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--launch-only", action="store_true")
ap.add_argument("--counters", default="")
args = ap.parse_args()
REPS, WARM = 20, 3
KERNELS = {   # candidate -> a substring of its kernel's name in the counter rows
    "f32": {"forward_camera": "cook_torrance_camera_kernel<1, 0, float, 4, false>", "forward_orthographic": "cook_torrance_kernel<1, 0, float, float, 4, false, true, false>",
            "backward_camera": "cook_torrance_camera_backward_kernel<1, 0, 2, float, false, false>", "backward_orthographic": "cook_torrance_backward_kernel<1, 0, 4, false, float, false>",
            "backward_params_camera": "cook_torrance_camera_backward_kernel<1, 0, 2, float, true, false>",
            "backward_params_orthographic": "cook_torrance_backward_kernel<1, 0, 2, false, float, true>"},
    "f16": {"forward_camera": "cook_torrance_camera_kernel<1, 0, __half, 4, true>", "forward_orthographic": "cook_torrance_kernel<1, 0, __half, float, 8, false, true, false>",
            "backward_camera": "cook_torrance_camera_backward_kernel<1, 0, 2, __half, false, false>", "backward_orthographic": "cook_torrance_backward_stream_kernel<1, 0",
            "backward_params_camera": "cook_torrance_camera_backward_kernel<1, 0, 2, __half, true, false>",
            "backward_params_orthographic": "cook_torrance_backward_kernel<1, 0, 2, false, __half, true>"},
}

if args.counters:
    # per kernel name: SQ_INSTS_VALU of one dispatch (the rows of a dispatch -- one per XCD -- summed), the median over its dispatches
    per = {}
    for path in glob.glob(os.path.join(args.counters, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if row["Counter_Name"] == "SQ_INSTS_VALU":
                d = per.setdefault(row["Kernel_Name"], {})
                d[row["Dispatch_Id"]] = d.get(row["Dispatch_Id"], 0.0) + float(row["Counter_Value"])
    rec = json.load(open(args.out))
    pixels = rec["size"] ** 2
    for r in rec["records"]:
        r["valu_instructions_per_pixel"] = {}
        for cand, needle in KERNELS[r["maps"]].items():
            hits = [statistics.median(v.values()) for k, v in per.items() if needle in k]
            if len(hits) == 1:
                r["valu_instructions_per_pixel"][cand] = round(hits[0] * 64 / pixels, 1)
    rec["counters"] = "rocprofv3 --pmc SQ_INSTS_VALU in a run of its own (--launch-only); wave instructions x 64 / pixels, the median over a kernel's dispatches"
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps([r["valu_instructions_per_pixel"] for r in rec["records"]], indent=1))
    sys.exit(0)

dev = torch.device("cuda", 0)
lib, stream = N.lib(), torch.cuda.current_stream(dev).cuda_stream
S = args.size


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
for dtype, tag in ((torch.float32, "f32"), (torch.float16, "f16")):
    maps = synth_material(S, dev, 3, dtype)
    kw = dict(light=[0.1, 0.1, 1.0], light_intensity=[1.0, 1.0, 1.0], light_type="point", light_size=1.0)
    out = torch.empty(1, 3, S, S, device=dev)
    cam = F.plan_cook_torrance(*maps, view_dir=[0.1, -0.2, 1.5], view_type="point", out=out, **kw)
    ortho = F.plan_cook_torrance(*maps, view_dir=[0.0, 0.0, 1.0], out=out, **kw)
    upstream = torch.rand(1, 3, S, S, device=dev)
    grads = [torch.empty_like(t) for t in maps]
    gp = torch.empty(9, device=dev)
    ws = torch.empty(max(lib.pbr_camera_backward_workspace_bytes(ctypes.byref(cam.desc)), lib.pbr_param_grad_workspace_bytes(ctypes.byref(ortho.desc))) // 8 + 1,
                     dtype=torch.float64, device=dev)
    gptr = [g.data_ptr() for g in grads] + [None]
    cands = {
        "forward_camera": lambda: N.check(lib.pbr_cook_torrance_camera(ctypes.byref(cam.desc), stream)),
        "forward_orthographic": lambda: N.check(lib.pbr_cook_torrance(ctypes.byref(ortho.desc), stream)),
        "backward_camera": lambda: N.check(lib.pbr_cook_torrance_camera_backward(ctypes.byref(cam.desc), upstream.data_ptr(), *gptr, None, None, stream)),
        "backward_orthographic": lambda: N.check(lib.pbr_cook_torrance_backward(ctypes.byref(ortho.desc), upstream.data_ptr(), *gptr, stream)),
        "backward_params_camera": lambda: N.check(lib.pbr_cook_torrance_camera_backward(ctypes.byref(cam.desc), upstream.data_ptr(), *gptr, gp.data_ptr(),
                                                                                        ws.data_ptr(), stream)),
        "backward_params_orthographic": lambda: N.check(lib.pbr_cook_torrance_backward_params(ctypes.byref(ortho.desc), upstream.data_ptr(), *gptr, gp.data_ptr(),
                                                                                              ws.data_ptr(), stream)),
    }
    if args.launch_only:
        for fn in cands.values():
            fn()
            fn()
        torch.cuda.synchronize()
        continue
    t = dict(zip(cands, median_us(list(cands.values()))))
    rec = {"size": S, "maps": tag, "orthographic_kernel": ortho.kernel_name, "us": {k: round(v, 2) for k, v in t.items()},
           "camera_over_orthographic": {k: round(t[k + "_camera"] / t[k + "_orthographic"], 4) for k in ("forward", "backward", "backward_params")}}
    records.append(rec)
    print(json.dumps(rec), flush=True)
    del maps, out, cam, ortho, upstream, grads, ws
    torch.cuda.empty_cache()

if not args.launch_only:
    result = {"what": "perspective camera (csrc/ct_camera.hip) against the orthographic kernels of the same shape: %d^2 metallic material, one point light "
                      "(tools/camera_probe.py)" % S,
              "timing": "HIP events around single launches, %d warm-ups, median of %d, the candidates alternating in one process" % (WARM, REPS),
              "size": S, "device": torch.cuda.get_device_name(0), "stamp": N.build_stamp(), "records": records}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
