#!/usr/bin/env python3
"""Do two builds give the same bytes from the light-stack entry points?  The step kernels add in a fixed order, so with the same kernels
(tools/isa_digests.py) equal arguments give equal bytes -- and a wrong pick or a wrong argument on the host side (PGRAD, map dtype, pixels per
lane, light type, workflow, a stride, the rows' offset, the count) does not.  For each case the SHA-256 of the loss, of every map gradient and
of the parameter-gradient block (the twelve loss steps, through functional._plan_and_launch), and of the stack (the three forward entry
points, through functional.cook_torrance_stack).  The cases are the smallest that reach every pick: B = 2, H = 5, W in {9, 12} (one pixel per
lane, a packed pair), L in {2, 3} (even, and odd: the per-shot kernel's last unpaired camera), fp32 and fp16 maps, directional and point
lights, metallic and specular workflow, weights as one plane per shot and as one shared plane, per-shot positions from the host and from a
device tensor (then the lights and intensities live on the device too).  Inputs come from a seeded CPU generator.

    python tools/stack_step_outputs.py --out A.json [--tree CHECKOUT]      # record: one build, one process (needs a ROCm device)
    python tools/stack_step_outputs.py --compare A.json B.json --out profiles/ab_NAME_outputs.json      # no device needed; status 1 if they differ"""
import argparse
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--tree", default=ROOT, help="the built checkout whose package is imported (default: this one)")
ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two recorded files instead of recording")
args = ap.parse_args()

if args.compare:
    a, b = (json.load(open(p)) for p in args.compare)
    da, db = a["digests"], b["digests"]
    differing = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    out = {"what": "tools/stack_step_outputs.py: SHA-256 of loss, map gradients, parameter gradients and stacks, two builds on the same device",
           "a": a["stamp"], "b": b["stamp"], "device": [a["device"], b["device"]], "cases": [len(da), len(db)],
           "tensors": [sum(len(v) for v in da.values()), sum(len(v) for v in db.values())], "differing": differing, "identical": not differing}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("identical: %s (%d cases, %d tensors)" % (out["identical"], len(da), out["tensors"][0]))
    sys.exit(0 if out["identical"] and da else 1)

import torch  # noqa: E402

sys.path.insert(0, os.path.abspath(args.tree))
from pypbr_amd import _native as N, functional as F  # noqa: E402

dev = torch.device("cuda", 0)
B, H = 2, 5
FAMILIES = (("", "directional"), ("camera_", "point"), ("view_", "point"))      # kind prefix, view_type


def sha(t):
    return None if t is None else hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def inputs(W, L, dtype, workflow, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, generator=g)
    normal = torch.cat([r(B, 2, H, W) - 0.5, r(B, 1, H, W) + 0.5], 1)
    maps = [r(B, 3, H, W), normal / normal.norm(dim=1, keepdim=True), r(B, 1, H, W) * 0.85 + 0.15,
            r(B, 1, H, W) if workflow == "metallic" else None, r(B, 3, H, W) if workflow == "specular" else None]
    lights = torch.cat([r(L, 2) - 0.5, r(L, 1) * 0.5 + 0.75], 1)
    cameras = lights * 0.9 + torch.tensor([0.02, -0.03, 0.4])
    return dict(maps=[None if t is None else t.to(dev, dtype) for t in maps], lights=lights, cameras=cameras, intens=r(L, 3) * 0.5 + 0.5,
                view=torch.tensor([0.05, 0.1, 0.9]), targets=r(B, L, 3, H, W).to(dev),
                weights={"per_shot": (r(B, L, 1, H, W) * 2.0).to(dev), "shared": (r(B, 1, 1, H, W) * 2.0).to(dev)})


digests = {}
before = dict(F.STACK_LAUNCHES)
for seed, (W, L, dtype, light_type, workflow) in enumerate(itertools.product((9, 12), (2, 3), (torch.float32, torch.float16), ("directional", "point"),
                                                                             ("metallic", "specular"))):
    x = inputs(W, L, dtype, workflow, 100 + seed)
    tag = "W%d_L%d_%s_%s_%s" % (W, L, str(dtype)[6:], light_type, workflow)
    for prefix, view_type in FAMILIES:
        kw = dict(light_type=light_type, light_size=1.0, view_type=view_type, albedo_is_srgb=True, return_srgb=True)
        view = {"": x["view"], "camera_": x["cameras"].mean(dim=0), "view_": x["cameras"]}[prefix]
        for where in ("host", "device") if prefix == "view_" else ("host",):
            params = tuple(t.to(dev) if where == "device" else t for t in (view, x["lights"], x["intens"]))
            with torch.no_grad():
                stack = F.cook_torrance_stack(*x["maps"], view_dir=params[0], light=params[1], light_intensity=params[2], **kw)
            digests["%s/%sforward/%s" % (tag, prefix, where)] = {"stack": sha(stack)}
            for fit, plane in itertools.product((False, True), (None, "per_shot", "shared")):
                kind = prefix + ("fit" if fit else "stack") + ("" if plane is None else "_w")
                weights = None if plane is None else x["weights"][plane]
                bufs, gp, loss = F._plan_and_launch(kind, x["maps"], kw, params, x["targets"], [True] * 5, weights)
                record = {"loss": sha(loss), "g_params": sha(gp)}
                record.update({"g_" + name: sha(b) for name, b in zip(("albedo", "normal", "roughness", "metallic", "specular"), bufs)})
                digests["%s/%s/%s/%s" % (tag, kind, plane, where)] = record
torch.cuda.synchronize()
took = {k: F.STACK_LAUNCHES[k] - before[k] for k in before}
assert all(took.values()) and len(took) == 15, took      # every one of the fifteen entry points was called
out = {"stamp": N.build_stamp(), "device": torch.cuda.get_device_name(0), "launches": took, "digests": digests}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
print("wrote %s: %d cases, %d tensors" % (args.out, len(digests), sum(len(v) for v in digests.values())))
