#!/usr/bin/env python3
"""MaterialAdam's projected update (csrc/adam.hip) at the sizes of a real fit: the 8 planes of a material (albedo 3, normal 3, roughness 1,
metallic 1) at 4096^2 and 1024^2, float32 and float16 maps (float16 with its float32 master).

  product     MaterialAdam.step(): one pbr_adam_step launch over the four maps, Python included;
  kernel      the same launch through the C ABI with the table built once: the kernel alone;
  policy N    the kernel built with -DPBR_ADAM_POLICY=N (`--build`, on the machine that has hipcc): bit 0 the parameter's load and store,
              bit 1 the gradient's load, bit 2 the loads of m, v, master, bit 3 their stores carry the non-temporal hint;
  fused       torch.optim.Adam(fused=True), where this torch build has it on the device, alone and followed by the projection written with
              ATen under no_grad (clamp_ per bounded map; clamp_ of z and F.normalize for the normal);
  default     torch.optim.Adam() (the foreach form), alone and followed by the same projection.
  float16 maps go to torch.optim.Adam as they are: it keeps no master copy, so its float16 rows move fewer bytes and compute something else.

Then the whole fit step at 256^2, L = 8 -- zero_grad, the stack loss (MultiLightRenderingLoss), backward, update -- eager and as the replay
of one captured graph, with MaterialAdam(capturable=True) and with torch.optim.Adam(capturable=True) + the ATen projection.

HIP events around the call, 3 warm-ups, the median of 20, the candidates alternating.  Bytes the update must move: 28 per float32 element,
30 per float16 element with its master; the fraction is of the MI355X's 8 TB/s.  Run by hand; not a test, asserts no duration.

    python tools/adam_probe.py --build
    python tools/adam_probe.py [--out profiles/adam_probe.json] [--sizes 4096,1024]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "pypbr_amd", "csrc")
POLICIES = (0, 8, 12, 14, 15)
HBM_PEAK = 8.0e12     # bytes / s, the MI355X's specification


def built_in_policy():
    """The library's own policy: the default of PBR_ADAM_POLICY in the source it was built from (None where the sources are not shipped)."""
    try:
        with open(os.path.join(CSRC, "adam.hip")) as f:
            m = re.search(r"#ifndef PBR_ADAM_POLICY\s+#define PBR_ADAM_POLICY (\d+)", f.read())
        return int(m.group(1)) if m else None
    except OSError:
        return None


def variant_path(policy):
    return os.path.join(ROOT, "tools", "libadam_policy%d.so" % policy)


def build_variants():
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-slp-vectorize", "-fno-gpu-rdc", "-Wno-unused-function"]
    jobs = [subprocess.Popen([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-DPBR_ADAM_POLICY=%d" % k, "-shared", os.path.join(CSRC, "adam.hip"),
                              "-o", variant_path(k)]) for k in POLICIES]
    if any(j.wait() for j in jobs):
        sys.exit("a variant did not build")
    print("built policies", POLICIES)


ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_probe.json"))
ap.add_argument("--sizes", default="4096,1024")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--step-size", type=int, default=256)
args = ap.parse_args()
if args.build:
    build_variants()
    sys.exit(0)

import torch  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402
from pypbr_amd.losses import MultiLightRenderingLoss  # noqa: E402
from pypbr_amd.materials import BasecolorMetallicMaterial  # noqa: E402
from pypbr_amd.optim import MaterialAdam, _coefficients, material_param_groups  # noqa: E402

assert torch.cuda.is_available(), "the probe measures on a ROCm device"
dev = torch.device("cuda", 0)
REPS, WARM = args.reps, 3
GROUPS = (("albedo", 3, dict(bounds=(0.0, 1.0))), ("normal", 3, dict(project="unit", min_z=0.0)), ("roughness", 1, dict(bounds=(0.05, 1.0))),
          ("metallic", 1, dict(bounds=(0.0, 1.0))))


def median_us(fns):
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


def maps(size, dtype, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for name, c, _ in GROUPS:
        t = torch.rand((c, size, size), device=dev, generator=gen) * 0.8 + 0.1
        if name == "normal":
            t = torch.nn.functional.normalize(t - torch.tensor([0.5, 0.5, 0.0], device=dev).view(3, 1, 1), dim=0)
        out.append(t.to(dtype).requires_grad_(True))
    for t in out:
        t.grad = ((torch.rand(t.shape, device=dev, generator=gen) - 0.5) * 1e-3).to(dtype)
    return out


def aten_projection(params):
    with torch.no_grad():
        for p, (name, _, kw) in zip(params, GROUPS):
            if kw.get("project") == "unit":
                p[2].clamp_(min=kw["min_z"])
                p.copy_(torch.nn.functional.normalize(p, dim=0))
            else:
                p.clamp_(*kw["bounds"])


def torch_adam(params, **kw):
    try:
        opt = torch.optim.Adam(params, lr=1e-3, **kw)
        opt.step()
        torch.cuda.synchronize()
        return opt, None
    except Exception as e:  # noqa: BLE001  (a torch build without the fused form on this device says so)
        return None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0])


def bare_call(fn, params, opt):
    """pbr_adam_step of one library over the optimiser's own state, the table built once."""
    table = (N.AdamTensor * len(params))()
    for i, (p, (name, c, kw)) in enumerate(zip(params, GROUPS)):
        st = opt.state[p]
        lo, hi = kw.get("bounds", (float("-inf"), float("inf")))
        kind = N.ADAM_UNIT if kw.get("project") == "unit" else N.ADAM_BOX
        table[i] = N.AdamTensor(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                st["master"].data_ptr() if "master" in st else None, p.shape[-1] * p.shape[-2], 0, p.stride(0), 0, p.grad.stride(0), 1, c,
                                N.F16 if p.dtype == torch.float16 else N.F32, kind, lo, hi, kw.get("min_z", float("-inf")), 0)
    coeffs = (N.AdamCoeffs * 1)(_coefficients(1e-3, (0.9, 0.999), 1e-8, 10))
    stream = torch.cuda.current_stream().cuda_stream

    def go():
        rc = fn(table, len(params), coeffs, None, 1, stream)
        assert rc == 0, rc
    return go


def entry_point(lib):
    fn = lib.pbr_adam_step
    fn.argtypes = N.lib().pbr_adam_step.argtypes
    fn.restype = ctypes.c_int
    return fn


records, notes = [], {}
for size in [int(v) for v in args.sizes.split(",")]:
    for dtype in (torch.float32, torch.float16):
        mine = maps(size, dtype, 1)
        opt = MaterialAdam([dict(params=[p], **kw) for p, (_, _, kw) in zip(mine, GROUPS)], lr=1e-3)
        opt.step()
        names, fns = ["product", "kernel"], [opt.step, bare_call(N.lib().pbr_adam_step, mine, opt)]
        for k in POLICIES:
            if os.path.exists(variant_path(k)):
                names.append("policy %d" % k)
                fns.append(bare_call(entry_point(ctypes.CDLL(variant_path(k))), mine, opt))
        for label, kw in (("fused", dict(fused=True)), ("default", dict())):
            theirs = maps(size, dtype, 2)
            adam, why = torch_adam(theirs, **kw)
            if adam is None:
                notes["torch.optim.Adam(%s) %s" % (label, str(dtype))] = "not available: " + why
                continue
            names += [label, label + " + ATen projection"]
            fns += [adam.step, (lambda a=adam, t=theirs: (a.step(), aten_projection(t)))]
        t = median_us(fns)
        elements = 8 * size * size
        per = 28 if dtype == torch.float32 else 30
        rec = {"grid": size, "maps": str(dtype).replace("torch.", ""), "planes": 8, "bytes_per_element": per,
               "time_us": {k: round(v, 1) for k, v in zip(names, t)},
               "kernel_fraction_of_hbm_peak": round(elements * per / (t[1] * 1e-6) / HBM_PEAK, 4),
               "product_fraction_of_hbm_peak": round(elements * per / (t[0] * 1e-6) / HBM_PEAK, 4)}
        for k in names[2:]:
            if not k.startswith("policy"):
                rec.setdefault("over_product", {})[k] = round(t[names.index(k)] / t[0], 2)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del mine, opt, fns
        torch.cuda.empty_cache()

# ---- the whole fit step at a small size: launch-bound, which is what the capture is for
S, L = args.step_size, 8
gen = torch.Generator().manual_seed(5)
lights = torch.stack([0.7 * torch.cos(torch.arange(L) * 0.785), 0.7 * torch.sin(torch.arange(L) * 0.785), torch.full((L,), 0.6)], dim=1)
KW = dict(view_dir=[0.0, 0.0, 1.0], light=lights, light_intensity=[1.0, 1.0, 1.0], light_type="point", light_size=1.0)


def material(seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.nn.functional.normalize(torch.rand(3, S, S, generator=g) - torch.tensor([0.5, 0.5, -0.5]).view(3, 1, 1), dim=0)
    return BasecolorMetallicMaterial(albedo=torch.rand(3, S, S, generator=g) * 0.8 + 0.1, normal=n, roughness=torch.rand(1, S, S, generator=g) * 0.6 + 0.2,
                                     metallic=torch.rand(1, S, S, generator=g) * 0.5).to(dev)


truth = material(7)
targets = F.cook_torrance_stack(*[truth.__dict__["_store"][k] for k in ("albedo", "normal", "roughness", "metallic")], **KW)
loss_fn = MultiLightRenderingLoss(light_type="point", view_dir=torch.tensor([0.0, 0.0, 1.0]), lights=lights, light_intensities=torch.tensor([1.0, 1.0, 1.0]),
                                  light_size=1.0)


def fit_routes(route):
    mat = material(8)
    groups = material_param_groups(mat, lr=1e-3)
    if route == "MaterialAdam":
        opt = MaterialAdam(groups, capturable=True)
        project = None
    else:
        opt = torch.optim.Adam([dict(params=g["params"], lr=g["lr"]) for g in groups], capturable=True)

        def project():
            with torch.no_grad():
                for g in groups:
                    p = g["params"][0]
                    if g.get("project") == "unit":
                        p[2].clamp_(min=g["min_z"])
                        p.copy_(torch.nn.functional.normalize(p, dim=0))
                    elif g.get("bounds") is not None:
                        p.clamp_(*g["bounds"])

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(mat, targets)
        loss.backward()
        opt.step()
        if project is not None:
            project()
        return loss
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    eager = median_us([step])[0]
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    replay = median_us([graph.replay])[0]
    return {"eager_us": round(eager, 1), "graph_replay_us": round(replay, 1)}


whole = {"grid": S, "lights": L, "MaterialAdam": fit_routes("MaterialAdam"), "torch.optim.Adam(capturable) + ATen projection": fit_routes("aten")}
print(json.dumps(whole), flush=True)

out = {"what": "the projected Adam update of a material's 8 planes (csrc/adam.hip, pypbr_amd.optim.MaterialAdam) against torch.optim.Adam, fused and "
               "default, alone and followed by the projection written with ATen; the kernel under each cache policy; the whole fit step (L = 8 stack loss "
               "+ update) eager and as a graph replay (tools/adam_probe.py)",
       "timing": "HIP events around the call, %d warm-ups, median of %d, the candidates alternating in one process" % (WARM, REPS),
       "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0), "stamp": N.build_stamp(), "policy_built_in": built_in_policy(),
       "notes": notes, "update": records, "whole_step": whole}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
