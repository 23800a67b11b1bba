#!/usr/bin/env python3
"""A/B of whole source REVISIONS in one process on one box: each revision is a copy of the
package built at a side path (`tools/ab_revisions.sh` extracts `git archive REV pypbr_amd include` to
tools/bin/REV/ and runs its own Makefile), imported here under an alias so that every revision fills ITS OWN
descriptor layout with ITS OWN host code and launches ITS OWN libpbr_hip.so.  All revisions see the same input
tensors; rounds are interleaved (rev A, rev B, rev C, rev A, ...) so that clock / box drift hits all alike.

    python tools/ab_revisions.py --revs r2=tools/bin/8600504,pre5=tools/bin/1dbff36,head=. \
        --cases headline,backward,config4 --rounds 7 --launches 500 --out profiles/r04_ab_revisions.json

After the settle launches of a case every output buffer of every revision is hashed; the case records whether all revisions agree
bit for bit (`bit_identical`, and which outputs of which alias differ).  `--rounds 0` stops there: digests only.  `--cases` also
takes the groups `digests` (the smallest shapes that reach each body of the render's chain rule: one-, two- and four-pixel lanes,
several lights, light / view adjoints, the streamed kernels, loss / stack / fit steps, the fused blend, tiled maps; three workflows,
both light types) and `chain_rule` (those kernels at the shapes tools/run_kernels.py times them at).  With `--spread-of a,b` -- ONE
revision under two aliases -- the run measures the spread of identical code itself (the larger of the two aliases' round ranges)
and reports for every other revision whether its median lies within it.

    python tools/ab_revisions.py --revs par=tools/bin/REV,par2=tools/bin/REV,head=. --spread-of par,par2 --cases chain_rule
    python tools/ab_revisions.py --revs par=tools/bin/REV,head=. --cases digests --rounds 0 --settle 2
"""
import argparse
import ctypes
import hashlib
import importlib.util
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_material  # noqa: E402


def load_revision(alias, path):
    pkg_dir = os.path.join(os.path.abspath(path), "pypbr_amd")
    name = "pypbr_rev_" + alias
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    F = importlib.import_module(name + ".functional")
    N = importlib.import_module(name + "._native")
    if hasattr(F, "USE_TORCH_OPS"):
        F.USE_TORCH_OPS = False                       # the registered operators exist once per process: every revision through its ctypes plan
    lib = N.lib()
    sha = hashlib.sha256(open(N.LIB_PATH, "rb").read()).hexdigest()[:16]
    return dict(alias=alias, F=F, N=N, lib=lib, lib_path=os.path.relpath(N.LIB_PATH, ROOT), lib_sha256_16=sha, abi=lib.pbr_abi_version())


def shared(sets, key, make):
    """Tensors every revision uses -- inputs AND outputs: where a buffer lies decides a memory-bound kernel's time by a few per cent
    (the same library under two aliases with buffers of its own each: 201.8 against 206.8 us), so all revisions run on the same addresses."""
    if key not in sets:
        sets[key] = make()
    return sets[key]


def build_case(case, rev, sets, dev):
    """-> (launch(i), kernel name, bytes per launch, output buffers) for this revision on the shared input tensors."""
    F, N, lib = rev["F"], rev["N"], rev["lib"]
    stream = torch.cuda.current_stream(dev).cuda_stream
    if case in ("headline", "backward"):
        kw = dict(view_dir=[0, 0, 1], light=[0.1, 0.1, 1.0], light_intensity=[1, 1, 1], light_type="point", light_size=1.0)
        plans = []
        for *packed, out in shared(sets, "packed4096", lambda: [F.pack_maps(*s, reserve_output=True) for s in sets["one4096"]]):
            plans.append(F.plan_cook_torrance(*packed, out=out, **kw))
        if case == "headline":
            fn = lib.pbr_cook_torrance
            return (lambda i: fn(ctypes.byref(plans[i % len(plans)].desc), stream)), plans[0].kernel_name, 44 * 4096 * 4096, [pl.out for pl in plans]
        g = shared(sets, "upstream4096", lambda: torch.rand(1, 3, 4096, 4096, device=dev))
        grads = shared(sets, "grads4096", lambda: [torch.empty(1, c, 4096, 4096, device=dev) for c in (3, 3, 1, 1)])
        ptrs = [t.data_ptr() for t in grads] + [None]
        fn = lib.pbr_cook_torrance_backward
        return (lambda i: fn(ctypes.byref(plans[i % len(plans)].desc), g.data_ptr(), *ptrs, stream)), "backward:" + plans[0].kernel_name, 76 * 4096 * 4096, grads
    if case in ("backward_f16", "loss_f16"):              # the streamed kernels of the fp16-map family
        kw = dict(view_dir=[0, 0, 1], light=[0.1, 0.1, 1.0], light_intensity=[1, 1, 1], light_type="point", light_size=1.0)
        maps = shared(sets, "half4096", lambda: [t.half() for t in sets["one4096"][0]])
        plan = F.plan_cook_torrance(*maps, **kw)
        g = shared(sets, "upstream4096", lambda: torch.rand(1, 3, 4096, 4096, device=dev))
        grads = shared(sets, "grads4096h", lambda: [torch.empty(1, c, 4096, 4096, device=dev, dtype=torch.float16) for c in (3, 3, 1, 1)])
        ptrs = [t.data_ptr() for t in grads] + [None]
        keep = (maps, g, grads)
        if case == "backward_f16":
            fn = lib.pbr_cook_torrance_backward
            return (lambda i, keep=keep: fn(ctypes.byref(plan.desc), g.data_ptr(), *ptrs, stream)), "backward fp16 maps", 44 * 4096 * 4096, grads
        loss = shared(sets, "loss", lambda: torch.empty((), device=dev))
        need = lib.pbr_mse_step_workspace_bytes(ctypes.byref(plan.desc))
        ws = shared(sets, "loss_ws", lambda: torch.empty(max(1, need // 4), device=dev))
        assert ws.numel() * 4 >= need, "revisions ask for different workspace sizes: %d bytes shared, %s needs %d" % (ws.numel() * 4, rev["alias"], need)
        fn = lib.pbr_cook_torrance_mse_step
        return (lambda i, keep=keep: fn(ctypes.byref(plan.desc), g.data_ptr(), *ptrs, loss.data_ptr(), ws.data_ptr(), stream)), "loss step fp16 maps", 44 * 4096 * 4096, grads + [loss]
    if case == "config4":
        kw = dict(view_dir=[0, 0, 1], light=[0.1, 0.1, 1.0], light_intensity=[1, 1, 1], light_type="point", light_size=1.0)
        plan = F.plan_cook_torrance(*sets["b64_1024"], out=shared(sets, "out_b64", lambda: torch.empty(64, 3, 1024, 1024, device=dev)), **kw)
        fn = lib.pbr_cook_torrance
        return (lambda i: fn(ctypes.byref(plan.desc), stream)), plan.kernel_name, 44 * 64 * 1024 * 1024, [plan.out]
    if case in CHAIN_CASES:
        return chain_case(case, rev, dev)
    raise SystemExit("unknown case " + case)


# ---- the kernels that differentiate the render (the chain rule of csrc/ct_chain_rule.hpp), one case per body / family.
# kind: backward | params (with the light / view gradients) | loss (mse step) | stack | fit (stack step with light / view gradients) |
#       folded (tiled maps) | blend;  shape (B, H, W) of the MAPS;  wf: metallic | specular | converted;  L lights of `light` type.
def _c(kind, shape, wf="metallic", light="point", L=1, f16=False, tile=1):
    return dict(kind=kind, shape=shape, wf=wf, light=light, L=L, f16=f16, tile=tile)


_BIG, _HALF = (1, 4096, 4096), (1, 2048, 2048)                 # the shapes tools/run_kernels.py times these kernels at
TIMED_CASES = {
    "backward_dir": _c("backward", _BIG, light="directional"), "backward_l4": _c("backward", _BIG, L=4),
    "tiled_bwd": _c("folded", _HALF, tile=2), "tiled_bwd_dir": _c("folded", _HALF, light="directional", tile=2),
    "blend_bwd": _c("blend", _BIG), "blend_bwd_tiled": _c("blend", _HALF, tile=2),
    "loss_f32": _c("loss", _BIG), "stack_l4": _c("stack", _BIG, L=4),
    "params_1023": _c("params", (64, 1024, 1023)),            # odd width with light / view adjoints: a one-pixel body
    "px1_converted": _c("backward", (64, 4096, 3), wf="converted"),                                   # rows shorter than four pixels: the one-pixel
    "px1_converted_dir": _c("backward", (64, 4096, 3), wf="converted", light="directional"),          # fp32 bodies without the adjoints
}
# Digest cases: the smallest shapes that reach each body, two materials; every family meets the three workflows and both light types.
_W = ("metallic", "specular", "converted")
DIGEST_CASES = {}
for _i, _wf in enumerate(_W):
    _lt, _lo = ("point", "directional")[_i % 2], ("directional", "point")[_i % 2]
    DIGEST_CASES.update({
        "d_px1_" + _wf: _c("backward", (2, 5, 3), _wf, _lt), "d_v4_" + _wf: _c("backward", (2, 4, 8), _wf, _lo),
        "d_v4_f16_" + _wf: _c("backward", (2, 4, 8), _wf, _lt, f16=True), "d_l3_" + _wf: _c("backward", (2, 4, 8), _wf, _lo, L=3),
        "d_pg_w6_" + _wf: _c("params", (2, 4, 6), _wf, _lt), "d_pg_w5_" + _wf: _c("params", (2, 4, 5), _wf, _lo),
        "d_pg_l3_" + _wf: _c("params", (2, 4, 6), _wf, _lt, L=3),
        "d_stream_bwd_" + _wf: _c("backward", (2, 2, 128), _wf, _lo, f16=True), "d_stream_loss_" + _wf: _c("loss", (2, 2, 128), _wf, _lt, f16=True),
        "d_loss_" + _wf: _c("loss", (2, 4, 8), _wf, _lo), "d_loss_l3_" + _wf: _c("loss", (2, 4, 8), _wf, _lt, L=3),
        "d_stack_l3_" + _wf: _c("stack", (2, 4, 8), _wf, _lo, L=3), "d_fit_l3_" + _wf: _c("fit", (2, 4, 8), _wf, _lt, L=3),
        "d_blend_" + _wf: _c("blend", (2, 4, 8), _wf, _lo),
        "d_tiled_" + _wf: _c("folded", (2, 8, 8), _wf, "point", tile=2), "d_tiled_dir_" + _wf: _c("folded", (2, 8, 8), _wf, "directional", tile=2),
        "d_tiled_f16_" + _wf: _c("folded", (2, 8, 8), _wf, _lt, f16=True, tile=2), "d_tiled_l3_" + _wf: _c("folded", (2, 8, 8), _wf, _lo, L=3, tile=2),
        "d_tiled_loss_" + _wf: _c("loss", (2, 8, 8), _wf, _lt, tile=2), "d_tiled_loss_dir_" + _wf: _c("loss", (2, 8, 8), _wf, "directional", tile=2),
        "d_tiled_blend_" + _wf: _c("blend", (2, 8, 8), _wf, _lo, tile=2), "d_tiled_6x6_" + _wf: _c("folded", (2, 6, 6), _wf, _lt, tile=2),
    })
CHAIN_CASES = {**TIMED_CASES, **DIGEST_CASES}
CASE_GROUPS = {"chain_rule": ["backward", "backward_f16", "loss_f16"] + list(TIMED_CASES), "digests": list(DIGEST_CASES)}
_inputs = {}                                                   # case -> the input tensors every revision reads


def _chain_inputs(case, spec, dev):
    if case not in _inputs:
        (B, H, W), L, tile = spec["shape"], spec["L"], spec["tile"]
        g = torch.Generator(device=dev).manual_seed(sum(map(ord, case)))
        dtype = torch.float16 if spec["f16"] else torch.float32

        def material():
            nxy = torch.rand(B, 2, H, W, device=dev, generator=g) - 0.5
            n = torch.cat([nxy, torch.ones(B, 1, H, W, device=dev)], 1)
            a, r = torch.rand(B, 3, H, W, device=dev, generator=g), torch.rand(B, 1, H, W, device=dev, generator=g) * 0.95 + 0.05
            m, sp = torch.rand(B, 1, H, W, device=dev, generator=g), torch.rand(B, 3, H, W, device=dev, generator=g)
            maps = [a, n / n.norm(dim=1, keepdim=True), r] + ([None, sp] if spec["wf"] == "specular" else [m, None])
            return [None if t is None else t.to(dtype) for t in maps]
        images = (B, L, 3, tile * H, tile * W) if spec["kind"] in ("stack", "fit") else (B, 3, tile * H, tile * W)
        _inputs[case] = dict(maps=material(), maps2=material() if spec["kind"] == "blend" else None,
                             mask=torch.rand(B, 1, H, W, device=dev, generator=g),
                             image=torch.rand(images, device=dev, generator=g))       # the upstream gradient, or the loss's target(s)
    return _inputs[case]


def chain_case(case, rev, dev):
    F, N, lib = rev["F"], rev["N"], rev["lib"]
    spec, stream = CHAIN_CASES[case], torch.cuda.current_stream(dev).cuda_stream
    inp = _chain_inputs(case, spec, dev)
    maps, image, L, kind = inp["maps"], inp["image"], spec["L"], spec["kind"]
    small = case in DIGEST_CASES                               # digests: a slanted view and lights apart, so that no term vanishes
    pos = [[0.1 + 0.25 * i, 0.1 - 0.2 * i, 1.0] for i in range(L)] if spec["light"] == "point" else [[0.3 - 0.2 * i, -0.2 + 0.15 * i, 1.0] for i in range(L)]
    kw = dict(view_dir=[0.15, -0.1, 1.0] if small else [0, 0, 1], light=pos if L > 1 else pos[0], light_type=spec["light"],
              light_intensity=[[1.0 / L if kind not in ("stack", "fit") else 1.0] * 3] * L if L > 1 else [1, 1, 1])
    if spec["light"] == "point":
        kw["light_size"] = 1.0
    if kind == "blend":
        kw["blend"] = tuple(inp["maps2"]) + (inp["mask"],)
    kw["out"] = shared(inp, "out", lambda: torch.empty((image.shape[0], 3) + tuple(image.shape[-2:]), device=dev))
    plan = F.plan_cook_torrance(*maps, tile=spec["tile"], convert_to_diffuse_specular=spec["wf"] == "converted", **kw)
    d = ctypes.byref(plan.desc)

    def like(key, t):                                          # outputs are the case's, not the revision's (see `shared`)
        return shared(inp, key, lambda: None if t is None else torch.empty_like(t))
    grads = [like("g%d" % i, t) for i, t in enumerate(maps)]
    gp = [g.data_ptr() if g is not None else None for g in grads]
    loss, g_params = like("loss", torch.empty((), device=dev)), like("g_params", torch.empty(3 + 6 * L, device=dev))
    outs = [g for g in grads if g is not None]

    def workspace(size_fn):                                    # shared like the outputs; a revision that needs more than the first one got stops here
        need = size_fn(d)
        ws = shared(inp, "ws", lambda: torch.empty(max(1, need // 8 + 1), dtype=torch.float64, device=dev))
        assert ws.numel() * 8 >= need, "revisions ask for different workspace sizes: %d bytes shared, %s needs %d" % (ws.numel() * 8, rev["alias"], need)
        return ws
    if kind == "backward":
        ws, fn, args = None, lib.pbr_cook_torrance_backward, (d, image.data_ptr(), *gp, stream)
    elif kind == "params":
        ws = workspace(lib.pbr_param_grad_workspace_bytes)
        fn, args, outs = lib.pbr_cook_torrance_backward_params, (d, image.data_ptr(), *gp, g_params.data_ptr(), ws.data_ptr(), stream), outs + [g_params]
    elif kind == "loss":
        ws = workspace(lib.pbr_mse_step_workspace_bytes)
        fn, args, outs = lib.pbr_cook_torrance_mse_step, (d, image.data_ptr(), *gp, loss.data_ptr(), ws.data_ptr(), stream), outs + [loss]
    elif kind == "stack":
        ws = workspace(lib.pbr_mse_stack_fit_workspace_bytes)
        fn, args, outs = lib.pbr_cook_torrance_mse_stack_step, (d, image.data_ptr(), *gp, loss.data_ptr(), ws.data_ptr(), stream), outs + [loss]
    elif kind == "fit":
        ws = workspace(lib.pbr_mse_stack_fit_workspace_bytes)
        fn, args = lib.pbr_cook_torrance_mse_stack_fit_step, (d, image.data_ptr(), *gp, g_params.data_ptr(), loss.data_ptr(), ws.data_ptr(), stream)
        outs = outs + [g_params, loss]
    elif kind == "folded":
        ws = workspace(lib.pbr_backward_folded_workspace_bytes)
        fn, args = lib.pbr_cook_torrance_backward_folded, (d, image.data_ptr(), *gp, ws.data_ptr(), stream)
    else:                                                      # blend: the plan's own launch works out the blended normal's sign first
        plan.launch(stream)
        grads2, g_mask = [like("h%d" % i, t) for i, t in enumerate(inp["maps2"])], like("g_mask", inp["mask"])
        G1, G2 = N.MapGrads(*gp), N.MapGrads(*[g.data_ptr() if g is not None else None for g in grads2])
        bd = N.BlendDesc.from_buffer_copy(plan._blend)
        bd.sign_mode = N.BLEND_SIGN_GIVEN
        ws = (G1, G2, bd, grads2)
        fn = lib.pbr_cook_torrance_blend_backward
        args = (d, ctypes.byref(bd), plan._workspace.data_ptr(), image.data_ptr(), ctypes.byref(G1), ctypes.byref(G2), g_mask.data_ptr(), stream)
        outs = outs + [g for g in grads2 if g is not None] + [g_mask]
    keep = (plan, inp, grads, ws)
    nbytes = sum(t.numel() * t.element_size() for t in [m for m in maps if m is not None] + [image] + outs)
    return (lambda i, keep=keep: fn(*args)), "%s %s %s L=%d%s" % (kind, spec["wf"], spec["light"], L, " fp16" if spec["f16"] else ""), nbytes, outs


def digest(t):
    return hashlib.sha256(t.detach().reshape(-1).contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--revs", required=True, help="alias=path[,alias=path...]; path holds pypbr_amd/ with its built libpbr_hip.so")
    ap.add_argument("--cases", default="headline,backward,config4")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--settle", type=int, default=400)
    ap.add_argument("--spread-of", default="", help="two aliases of ONE revision (a,b): their round ranges are the spread the others are held against")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    revs = [load_revision(*kv.split("=")) for kv in args.revs.split(",")]
    sets = {"one4096": [synth_material(4096, dev, 1234 + i) for i in range(3)]}
    one = synth_material(1024, dev, 99)
    sets["b64_1024"] = [torch.stack([t] * 64).contiguous() for t in one]
    for b in range(1, 64):                                  # distinct materials (cheap: perturb, keep ranges)
        sets["b64_1024"][0][b].mul_(1.0 - 0.005 * b)
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        head = os.environ.get("PBR_GIT_HEAD", "unknown")     # the GPU box has no .git: the caller passes it
    record = dict(tool="tools/ab_revisions.py", git_head=head, device=torch.cuda.get_device_name(0), rounds=args.rounds, launches=args.launches,
                  revisions=[{k: r[k] for k in ("alias", "lib_path", "lib_sha256_16", "abi")} for r in revs], cases=[])
    cases = [c for name in args.cases.split(",") for c in CASE_GROUPS.get(name, [name])]
    spread_of = [a for a in args.spread_of.split(",") if a]
    for case in cases:
        launchers = [build_case(case, r, sets, dev) for r in revs]
        # same values out of every revision: the revisions write the SAME buffers one after the other; after a revision's settle launches every
        # output is hashed (over a sentinel fill: an output a kernel fails to write must not agree by accident), and the case records whether
        # all revisions agree bit for bit
        digests = []
        for (launch, _, _, outs) in launchers:
            for t in outs:
                t.fill_(-7.0)
            for i in range(max(1, args.settle // len(launchers))):
                assert launch(i) == 0
            torch.cuda.synchronize()
            digests.append([digest(t) for t in outs])
        entry = dict(case=case, outputs=len(digests[0]), bit_identical=all(d == digests[0] for d in digests), results=[])
        if not entry["bit_identical"]:
            entry["differs"] = {r["alias"]: [i for i, (x, y) in enumerate(zip(d, digests[0])) if x != y] for r, d in zip(revs, digests) if d != digests[0]}
        for (launch, _, _, _) in launchers if args.rounds else []:      # hashing copied the outputs to the host: the clocks settle again, untimed
            for i in range(max(1, args.settle // len(launchers))):
                launch(i)
        times = [[] for _ in revs]
        for rnd in range(args.rounds):
            order = list(range(len(revs)))
            order = order[rnd % len(revs):] + order[:rnd % len(revs)]      # rotate who goes first
            for k in order:
                launch = launchers[k][0]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.launches):
                    launch(i)
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
        if not args.rounds:                                    # digests only
            print("%-22s %2d outputs  %s" % (case, entry["outputs"], "bit-identical" if entry["bit_identical"] else "DIFFERS " + json.dumps(entry["differs"])), flush=True)
            for r, d, (_, kname, _, _) in zip(revs, digests, launchers):
                entry["results"].append(dict(alias=r["alias"], kernel=kname, sha256_16=d))
            record["cases"].append(entry)
            continue
        base = statistics.median(times[-1])
        for r, t, d, (_, kname, nbytes, _) in zip(revs, times, digests, launchers):
            med = statistics.median(t)
            entry["results"].append(dict(alias=r["alias"], kernel=kname, us_rounds=[round(x, 2) for x in t], us_median=round(med, 2), sha256_16=d,
                                         us_min=round(min(t), 2), tb_per_s=round(nbytes / med / 1e6, 3), vs_last=round(med / base, 4)))
            print("%-9s %-6s median %8.2f us  min %8.2f  (%5.3f TB/s)  x%.4f of %s   %s" % (case, r["alias"], med, min(t), nbytes / med / 1e6, med / base,
                                                                                              revs[-1]["alias"], " ".join("%.1f" % x for x in t)), flush=True)
        if spread_of:
            # the run-to-run spread of IDENTICAL code, measured in this very run: the same revision under two aliases; the larger of their round
            # ranges.  Every other revision's median is held against the aliases' own medians: inside [lowest - spread, highest + spread] or not.
            same = [k for k, r in enumerate(revs) if r["alias"] in spread_of]
            spread = max(max(times[k]) - min(times[k]) for k in same)
            meds = [statistics.median(times[k]) for k in same]
            entry["spread_us"] = round(spread, 2)
            for k, r in enumerate(revs):
                if k not in same:
                    med = statistics.median(times[k])
                    entry["results"][k]["within_spread"] = bool(min(meds) - spread <= med <= max(meds) + spread)
            print("%-9s bit-identical %s   spread of %s: %.2f us   %s" % (case, entry["bit_identical"], "/".join(spread_of), spread,
                  "  ".join("%s %s" % (x["alias"], "inside" if x["within_spread"] else "OUTSIDE") for x in entry["results"] if "within_spread" in x)), flush=True)
        record["cases"].append(entry)
    print("bit-identical cases: %d of %d" % (sum(c["bit_identical"] for c in record["cases"]), len(record["cases"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
