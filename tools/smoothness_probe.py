#!/usr/bin/env python3
"""The smoothness prior (csrc/smoothness.hip, pypbr_amd.priors) at the sizes of a real fit: the four maps of a BasecolorMetallicMaterial
(albedo 3, normal 3, roughness 1, metallic 1 planes) with one shared weight plane, at 4096^2 and 1024^2, float32 and float16 maps, L2 and
Charbonnier.

  product     priors.smoothness(...) and .backward(): the one launch, the finish launch, autograd and Python included;
  kernel      pbr_smoothness_step through the C ABI with the table built once: the two launches alone;
  aten        the same definition written with ATen in THIS file (two shifted differences, squares, a channel sum, a square root, a
              weighted mean) and autograd's backward through it.

Then the whole fit step of tools/adam_probe.py at 256^2, L = 8 -- zero_grad, the stack loss + the prior, backward, MaterialAdam -- eager
and as the replay of one captured graph, with the product's prior and with the ATen prior.

HIP events around the call, 3 warm-ups, the median of 20 with the quartiles, the candidates alternating in one run.  Bytes the kernel must
move: every parameter read once, every gradient written once, the weights read once per entry -- 80 per pixel for this material in float32
(8 x 4 + 8 x 4 + 4 x 4), 48 in float16; the fraction is of the MI355X's 8 TB/s.  Run by hand; not a test, asserts no duration.

    python tools/smoothness_probe.py [--out profiles/smoothness_probe.json] [--sizes 4096,1024]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12     # bytes / s, the MI355X's specification

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoothness_probe.json"))
ap.add_argument("--sizes", default="4096,1024")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--step-size", type=int, default=256)
args = ap.parse_args()

import torch  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402
from pypbr_amd import priors  # noqa: E402
from pypbr_amd.losses import MultiLightRenderingLoss  # noqa: E402
from pypbr_amd.materials import BasecolorMetallicMaterial  # noqa: E402
from pypbr_amd.optim import MaterialAdam, material_param_groups  # noqa: E402

assert torch.cuda.is_available(), "the probe measures on a ROCm device"
dev = torch.device("cuda", 0)
REPS, WARM = args.reps, 3
CHANNELS = (3, 3, 1, 1)
LAMBDAS = (0.05, 0.02, 0.3, 0.3)
EPS = 1e-3


def timed(fns):
    """[(median, lower quartile, upper quartile)] in microseconds, the candidates alternating."""
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
    out = []
    for t in times:
        q = statistics.quantiles(t, n=4)
        out.append((statistics.median(t), q[0], q[2]))
    return out


def aten_prior(tensors, lambdas, kind, weights):
    """The definition as a user writes it (wrap off, "mean")."""
    total = None
    for p, lam in zip(tensors, lambdas):
        x = p.float()
        dx, dy = torch.zeros_like(x), torch.zeros_like(x)
        dx[..., :-1] = x[..., 1:] - x[..., :-1]
        dy[..., :-1, :] = x[..., 1:, :] - x[..., :-1, :]
        s = (dx * dx + dy * dy).sum(dim=0, keepdim=True)
        phi = s if kind == "l2" else torch.sqrt(s + EPS * EPS) - EPS
        term = lam * (weights * phi).mean()
        total = term if total is None else total + term
    return total


def maps(size, dtype, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return [(torch.rand((c, size, size), device=dev, generator=gen) * 0.8 + 0.1).to(dtype).requires_grad_(True) for c in CHANNELS]


def bare_call(tensors, weights, kind):
    grads = [torch.empty_like(t) for t in tensors]
    table = (N.SmoothTensor * len(tensors))(*[priors._entry(t.detach(), g, weights, priors._scale(lam, t, "mean"), priors.KINDS[kind], EPS, False)
                                              for t, g, lam in zip(tensors, grads, LAMBDAS)])
    lib = N.lib()
    nbytes = lib.pbr_smoothness_workspace_bytes(table, len(tensors))
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=dev)
    loss, terms = torch.empty((), device=dev), torch.empty(len(tensors), device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def go():
        rc = lib.pbr_smoothness_step(table, len(tensors), loss.data_ptr(), terms.data_ptr(), ws.data_ptr(), nbytes, stream)
        assert rc == 0, rc
    go.keep = (grads, ws, loss, terms)
    return go


def forward_backward(fn, tensors):
    def go():
        for t in tensors:
            t.grad = None
        fn().backward()
    return go


records = []
for size in [int(v) for v in args.sizes.split(",")]:
    weights = torch.rand((1, size, size), device=dev)
    for dtype in (torch.float32, torch.float16):
        for kind in ("l2", "charbonnier"):
            mine, theirs = maps(size, dtype, 1), maps(size, dtype, 1)
            names = ["product", "kernel", "aten"]
            fns = [forward_backward(lambda: priors.smoothness(mine, LAMBDAS, kind=kind, eps=EPS, weights=weights), mine),
                   bare_call(mine, weights, kind),
                   forward_backward(lambda: aten_prior(theirs, LAMBDAS, kind, weights), theirs)]
            fns[0](), fns[2]()
            scale = max(float(t.grad.abs().max()) for t in theirs)
            agree = max(float((a.grad.float() - b.grad.float()).abs().max()) for a, b in zip(mine, theirs)) / scale
            t = timed(fns)
            per = (2 * 8 + 4) * 4 if dtype == torch.float32 else 2 * 8 * 2 + 4 * 4
            rec = {"grid": size, "maps": str(dtype).replace("torch.", ""), "kind": kind, "planes": 8, "bytes_per_pixel": per,
                   "time_us": {k: {"median": round(v[0], 1), "q1": round(v[1], 1), "q3": round(v[2], 1)} for k, v in zip(names, t)},
                   "kernel_fraction_of_hbm_peak": round(size * size * per / (t[1][0] * 1e-6) / HBM_PEAK, 4),
                   "aten_over_product": round(t[2][0] / t[0][0], 2),
                   "aten_over_product_range": [round(t[2][1] / t[0][2], 2), round(t[2][2] / t[0][1], 2)],
                   "gradients_max_difference_over_max_gradient": agree}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del mine, theirs, fns
            torch.cuda.empty_cache()

# ---- the whole fit step at a small size: launch-bound, which is what the capture is for (tools/adam_probe.py's step + the prior)
S, L = args.step_size, 8
lights = torch.stack([0.7 * torch.cos(torch.arange(L) * 0.785), 0.7 * torch.sin(torch.arange(L) * 0.785), torch.full((L,), 0.6)], dim=1)
KW = dict(view_dir=[0.0, 0.0, 1.0], light=lights, light_intensity=[1.0, 1.0, 1.0], light_type="point", light_size=1.0)
NAMES = ("albedo", "normal", "roughness", "metallic")


def material(seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.nn.functional.normalize(torch.rand(3, S, S, generator=g) - torch.tensor([0.5, 0.5, -0.5]).view(3, 1, 1), dim=0)
    return BasecolorMetallicMaterial(albedo=torch.rand(3, S, S, generator=g) * 0.8 + 0.1, normal=n, roughness=torch.rand(1, S, S, generator=g) * 0.6 + 0.2,
                                     metallic=torch.rand(1, S, S, generator=g) * 0.5).to(dev)


truth = material(7)
targets = F.cook_torrance_stack(*[truth.__dict__["_store"][k] for k in NAMES], **KW)
loss_fn = MultiLightRenderingLoss(light_type="point", view_dir=torch.tensor([0.0, 0.0, 1.0]), lights=lights, light_intensities=torch.tensor([1.0, 1.0, 1.0]),
                                  light_size=1.0)
step_weights = torch.rand((1, S, S), device=dev)


def fit_routes(route):
    mat = material(8)
    groups = material_param_groups(mat, lr=1e-3)
    opt = MaterialAdam(groups, capturable=True)
    store = mat.__dict__["_store"]
    if route == "none":
        prior = None
    elif route == "product":
        module = priors.MaterialSmoothness(dict(zip(NAMES, LAMBDAS)), eps=EPS)
        prior = lambda: module(mat, weights=step_weights)                          # noqa: E731
    else:
        prior = lambda: aten_prior([store[k] for k in NAMES], LAMBDAS, "charbonnier", step_weights)     # noqa: E731

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(mat, targets)
        if prior is not None:
            loss = loss + prior()
        loss.backward()
        opt.step()
        return loss
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    eager = timed([step])[0]
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    replay = timed([graph.replay])[0]
    return {"eager_us": {"median": round(eager[0], 1), "q1": round(eager[1], 1), "q3": round(eager[2], 1)},
            "graph_replay_us": {"median": round(replay[0], 1), "q1": round(replay[1], 1), "q3": round(replay[2], 1)}}


whole = {"grid": S, "lights": L, "no prior": fit_routes("none"), "MaterialSmoothness": fit_routes("product"), "ATen prior": fit_routes("aten")}
for key in ("eager_us", "graph_replay_us"):
    whole["aten_over_product_" + key] = round(whole["ATen prior"][key]["median"] / whole["MaterialSmoothness"][key]["median"], 2)
print(json.dumps(whole), flush=True)

out = {"what": "the smoothness prior of a material's 8 planes with one shared weight plane (csrc/smoothness.hip, pypbr_amd.priors.smoothness), forward + "
               "backward, against the same definition written with ATen and autograd; the kernel alone; the whole fit step (L = 8 stack loss + prior + "
               "MaterialAdam) eager and as a graph replay (tools/smoothness_probe.py)",
       "timing": "HIP events around the call, %d warm-ups, median and quartiles of %d, the candidates alternating in one process" % (WARM, REPS),
       "hbm_peak_bytes_per_s": HBM_PEAK, "device": torch.cuda.get_device_name(0), "stamp": N.build_stamp(),
       "prior": records, "whole_step": whole}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
