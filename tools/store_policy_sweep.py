#!/usr/bin/env python3
"""Result-store policy of the forward render family: in-process A/B of several builds of libpbr_hip.so on the same tensors.

Every build has the same ABI and fills nothing itself: ONE descriptor per case (this tree's host code), launched through each library in turn.
The first library named is the yardstick (the parent commit's build); the others are alternative builds of the store policy
(`tools/build_alt.sh st2 -DPBR_RESULT_STORE=2`, ...: 0 plain, 1 hinted, 2 write-through, 3 write-through + hint).

Protocol (the project's A/B rule): settle launches first (300 for the 4096^2 case, else what fills 150 ms), then `--rounds` rounds; in a round
every library is timed once, the order rotated from round to round; a round's figure is the MEDIAN of `--samples` samples, a sample being
`--burst` back-to-back launches between two events (so that what happens between consecutive launches is inside the figure).  A build counts as
faster only when its median lies below the yardstick's by more than the yardstick's spread (max - min of its per-round figures) in the same run.

    python tools/store_policy_sweep.py --libs parent=PATH,hinted=pypbr_amd/libpbr_hip.so,plain=tools/bin/st0/libpbr_hip.so,... --out FILE.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_material  # noqa: E402
from pypbr_amd import _native as N, functional as F  # noqa: E402

POINT = dict(view_dir=[0, 0, 1], light=[0.1, 0.1, 1.0], light_intensity=[1, 1, 1], light_type="point", light_size=1.0)
DIRECTIONAL = dict(view_dir=[0, 0, 1], light=[0.3, -0.2, 1.0], light_intensity=[1, 1, 1], light_type="directional",
                   convert_to_diffuse_specular=True, specular_is_srgb=True)


def batch_of(size, batch, dev, seed, dtype=torch.float32):
    one = synth_material(size, dev, seed)
    maps = [torch.stack([t] * batch).contiguous() for t in one]
    for b in range(1, batch):
        maps[0][b].mul_(1.0 - 0.005 * b)
    return [t.to(dtype) for t in maps]


def build_case(case, dev):
    """-> list of plans (rotated launch by launch) on this tree's host code."""
    if case == "config2_4096":                       # bench.py config 2: arena layout, three rotating sets
        plans = []
        for i in range(3):
            *packed, out = F.pack_maps(*synth_material(4096, dev, 1234 + i), reserve_output=True)
            plans.append(F.plan_cook_torrance(*packed, out=out, **POINT))
        return plans
    if case == "config3_8x2048":                     # config 3's per-GPU share: directional, converted workflow
        return [F.plan_cook_torrance(*batch_of(2048, 8, dev, 31), **DIRECTIONAL)]
    if case == "config4_64x1024":                    # config 4's per-GPU share
        return [F.plan_cook_torrance(*batch_of(1024, 64, dev, 41), **POINT)]
    if case == "f16_4x4096":                         # the 8-pixel kernel: fp16 maps, fp32 result through the piece exchange
        return [F.plan_cook_torrance(*batch_of(4096, 4, dev, 51, torch.float16), **POINT)]
    if case == "repeat_2048_tile2":                  # repeat-inner: 134 MB of maps + 201 MB of result per step, two rotating sets (> 256 MiB each)
        return [F.plan_cook_torrance(*synth_material(2048, dev, 61 + i), tile=2, **POINT) for i in range(2)]
    if case.startswith("gen:"):                      # gen:BATCH:SIZE:point|directional:metallic|converted[:linear|:xcd6] -- which of shape, light and workflow decides
        _, batch, size, light, workflow, *order = case.split(":")
        kw = dict(POINT if light == "point" else {k: v for k, v in DIRECTIONAL.items() if k not in ("convert_to_diffuse_specular", "specular_is_srgb")})
        if workflow == "converted":
            kw.update(convert_to_diffuse_specular=True, specular_is_srgb=True)
        if order:                                     # ...:linear | ...:xcd6 -- the workgroup order forced (else the rule: schedule_xcd_log2)
            kw["schedule"] = N.SCHEDULE_LINEAR if order[0] == "linear" else N.schedule_xcd(int(order[0][3:]))
        if int(batch) == 1:
            plans = []
            for i in range(3):
                *packed, out = F.pack_maps(*synth_material(int(size), dev, 71 + i), reserve_output=True)
                plans.append(F.plan_cook_torrance(*packed, out=out, **kw))
            return plans
        return [F.plan_cook_torrance(*batch_of(int(size), int(batch), dev, 81), **kw)]
    raise SystemExit("unknown case " + case)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True, help="name=path[,name=path...]; the first is the yardstick")
    ap.add_argument("--cases", default="config2_4096,config3_8x2048,config4_64x1024,f16_4x4096,repeat_2048_tile2")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--burst", type=int, default=6)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    libs = []
    for kv in args.libs.split(","):
        name, path = kv.split("=")
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.pbr_cook_torrance.argtypes = [ctypes.POINTER(N.RenderDesc), ctypes.c_void_p]
        lib.pbr_cook_torrance.restype = ctypes.c_int
        lib.pbr_render_desc_size.restype = ctypes.c_size_t
        assert lib.pbr_render_desc_size() == ctypes.sizeof(N.RenderDesc) and lib.pbr_abi_version() == N.ABI_VERSION, "another ABI: " + path
        libs.append((name, lib))
    stream = torch.cuda.current_stream(dev).cuda_stream
    record = dict(tool="tools/store_policy_sweep.py", device=torch.cuda.get_device_name(0), rounds=args.rounds, samples=args.samples, burst=args.burst,
                  libs=[n for n, _ in libs], cases=[])
    for case in args.cases.split(","):
        plans = build_case(case, dev)
        refs = [ctypes.byref(p.desc) for p in plans]

        def launch(lib, i):
            rc = lib.pbr_cook_torrance(refs[i % len(refs)], stream)
            assert rc == 0, rc

        want = None
        for name, lib in libs:                       # same bits out of every build
            plans[0].result.fill_(float("nan"))
            launch(lib, 0)
            got = plans[0].result.clone()
            want = got if want is None else want
            assert torch.equal(got, want) and bool(torch.isfinite(got).all()), (case, name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(6):
            launch(libs[0][1], i)
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 6
        settle = 300 if case == "config2_4096" else max(30, int(150e3 / us) + 1)
        for i in range(settle):
            launch(libs[i % len(libs)][1], i)
        torch.cuda.synchronize()
        rounds = [[] for _ in libs]
        for rnd in range(args.rounds):
            order = list(range(len(libs)))
            order = order[rnd % len(libs):] + order[:rnd % len(libs)]
            if rnd % 2:
                order.reverse()
            for k in order:
                lib = libs[k][1]
                samples = []
                for s in range(args.samples):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(args.burst):
                        launch(lib, s * args.burst + i)
                    e1.record()
                    e1.synchronize()
                    samples.append(e0.elapsed_time(e1) * 1e3 / args.burst)
                rounds[k].append(statistics.median(samples))
        base_med = statistics.median(rounds[0])
        base_spread = max(rounds[0]) - min(rounds[0])
        entry = dict(case=case, kernel=plans[0].kernel_name, settle=settle, yardstick_spread_us=round(base_spread, 3), results=[])
        for (name, _), r in zip(libs, rounds):
            med = statistics.median(r)
            verdict = "yardstick" if r is rounds[0] else ("faster" if med < base_med - base_spread else ("slower" if med > base_med + base_spread else "inside the spread"))
            entry["results"].append(dict(lib=name, us_median=round(med, 3), us_min=round(min(r), 3), us_max=round(max(r), 3), spread_us=round(max(r) - min(r), 3),
                                         vs_yardstick=round(med / base_med, 5), verdict=verdict, us_rounds=[round(x, 2) for x in r]))
            print("%-18s %-30s %-15s median %9.3f us  spread %6.3f  x%.4f  %s" % (case, plans[0].kernel_name, name, med, max(r) - min(r), med / base_med, verdict), flush=True)
        record["cases"].append(entry)
        del plans, refs, want
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
