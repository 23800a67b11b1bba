"""Material export (csrc/pack_image.hip): pbr_pack_images on one 3-plane SIZE^2 fp32 map in 8 bit (12 B in, 3 B out per texel) and on a
5-map 1024^2 material, each against the ATen sequence t.mul(255).byte().permute(1, 2, 0).contiguous() on the same device; then the
whole to_pil() of a device-resident material against the upstream route (.cpu() per map, then the host arithmetic).  HIP events around
each device call, wall clock around the calls that end on the host; 3 warm-ups, the median of 20.  Prints one JSON object per line.
    python tools/export_probe.py [SIZE=4096]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPS = 3, 20


def median_us(fn, wall=False):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        if wall:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6)
            continue
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return sorted(times)[len(times) // 2]


def aten_samples(t, normal=False):
    if normal:
        t = (t + 1.0) * 0.5
    return t.mul(255).byte().permute(1, 2, 0).contiguous()


def upstream_to_pil(maps):
    """base.py:793-850 for 8-bit modes: .cpu() per map, then torchvision's to_pil_image arithmetic on the host."""
    from PIL import Image
    out = {}
    for name, t in maps.items():
        if name == "normal":
            t = (t + 1.0) * 0.5
        t = t.cpu()
        a = t.mul(255).byte().numpy().transpose(1, 2, 0)
        out[name] = Image.fromarray(np.ascontiguousarray(a[:, :, 0] if a.shape[2] == 1 else a))
    return out


def material_maps(size, g):
    n = torch.randn(3, size, size, generator=g)
    n = n / n.norm(dim=0, keepdim=True)
    return {"albedo": torch.rand(3, size, size, generator=g).cuda(), "normal": n.cuda(), "roughness": torch.rand(1, size, size, generator=g).cuda(),
            "height": torch.rand(1, size, size, generator=g).cuda(), "metallic": torch.rand(1, size, size, generator=g).cuda()}


def main():
    from pypbr_amd import _upload as U, functional as F
    from pypbr_amd.materials import BasecolorMetallicMaterial
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    g = torch.Generator().manual_seed(1)

    def report(what, size, us, nbytes=None):
        rec = {"what": what, "size": size, "median_us": round(us, 1)}
        if nbytes is not None:
            rec.update(bytes=nbytes, tb_per_s=round(nbytes / us / 1e6, 3), of_8_tb_per_s=round(nbytes / us / 1e6 / 8.0, 3))
        print(json.dumps(rec), flush=True)

    t = torch.rand(3, S, S, generator=g).cuda()
    out = torch.empty(S, S, 3, dtype=torch.uint8, device="cuda")
    assert torch.equal(F.pack_image(t, out=out), aten_samples(t))
    report("pack_images, 3 planes -> RGB uint8", S, median_us(lambda: F.pack_image(t, out=out)), 15 * S * S)
    report("aten mul(255).byte().permute.contiguous, 3 planes", S, median_us(lambda: aten_samples(t)))
    del t, out

    maps = material_maps(1024, g)
    px = 1024 * 1024
    outs = {k: torch.empty(1024, 1024, v.shape[0], dtype=torch.uint8, device="cuda") for k, v in maps.items()}
    rows = [U._image_pack(maps[k], outs[k].data_ptr(), 8, k == "normal") for k in maps]
    dev = maps["albedo"].device
    report("pack_images, 5-map material (9 planes), one launch", 1024, median_us(lambda: U._pack_images_call(dev, rows, 1024, 1024)), 9 * 5 * px)
    report("aten sequence per map, 5-map material", 1024, median_us(lambda: [aten_samples(v, k == "normal") for k, v in maps.items()]))
    for k, v in maps.items():
        assert torch.equal(outs[k], aten_samples(v, k == "normal")), k

    for size in (1024, S):
        m = BasecolorMetallicMaterial(**material_maps(size, g))
        assert m.device.type == "cuda"
        ours, theirs = m.to_pil(), upstream_to_pil(m._raw)
        assert all(np.array_equal(np.array(ours[k]), np.array(theirs[k])) for k in ours)
        report("to_pil() of a device-resident 5-map material, this build (wall clock)", size, median_us(m.to_pil, wall=True))
        report("to_pil() the upstream route: .cpu() per map + host arithmetic (wall clock)", size, median_us(lambda: upstream_to_pil(m._raw), wall=True))
        report("download_samples alone: the launch + the one copy (wall clock)", size, median_us(lambda: F.download_samples(m._raw, 8), wall=True))
        del m


if __name__ == "__main__":
    main()
