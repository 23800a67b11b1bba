"""Writes tests/golden/packing.npz: what the REAL reference's MaterialBase.from_tensor and MaterialBase.as_tensor
(pypbr/materials/base.py:319-487) make of packed tensors, and upstream autograd's gradients through from_tensor -- the fixture of
tests/test_gpu_packing.py and tests/test_packing_host.py.  Development container only: it imports the reference through
oracle/ref_import.import_reference() (nothing under oracle/ is changed).

Only float arrays are stored (the float64 gradients as float64); the torch version and the ATen thread count they were made with are
stored as float arrays too (meta_torch as the version's bytes, meta_threads).  The packed inputs hold multiples of 1/255 so that the file
stays small; the near-circle set and nothing else holds arbitrary floats.  The `is_normalized` inputs are `normalized(t)` = t * 2 - 1 of
the stored ones (one IEEE product and difference: the same floats on every machine), so they are not stored.

    python tools/gen_packing_golden.py [OUT_DIR]        (default: tests/golden)

Keys (size = "37x53" ...; mode "u" = is_normalized False, "n" = True; cls = "metallic" | "specular"):
  in__<size>                         the packed 9-channel input; LAYOUTS says which of its channels a layout takes
  ft__<cls>__<layout>__<mode>__<size>__<map>     from_tensor's maps
  nc_in, nc_out__<mode>              pairs with |1 - s| < 5e-4 on both sides of the clamp, and from_tensor's normal map of them
  at__<size>__<case>                 as_tensor of the material from_tensor makes of in__<size> under layout "full9": AS_CASES
  g_in__<layout>, g_w__<layout>__<map>           gradient inputs (every pair |1 - s| >= 1e-2, clamped and unclamped ones) and weights
  g64__<layout>__<mode>, g32__<layout>__<mode>   upstream autograd of sum(w * maps) w.r.t. the packed tensor in float64 and in float32
  meta_grad_envelope                 the largest |g32 - g64| / max(1, |g64|) over all of them: upstream's own fp32 error
At generation time the tool asserts that a numpy fp32 restatement of the kernel's operation order (csrc/packing.hip) is within 1e-6 of
every 2-channel normal it stores, the near-circle set included: the tolerance of the GPU test is attainable.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
THREADS = 8
SIZES = ((1, 1), (1, 17), (5, 1), (37, 53))
# layout -> (first channel of in__<size> it starts at, [(map, channels), ...])
LAYOUTS = {
    "rgbn8": (0, [("albedo", 3), ("normal", 3), ("roughness", 1), ("metallic", 1)]),
    "full9": (0, [("albedo", 3), ("normal", 2), ("roughness", 1), ("metallic", 1), ("height", 1), ("opacity", 1)]),
    "xy2": (3, [("normal", 2)]),
}
CLASSES = {"metallic": "BasecolorMetallicMaterial", "specular": "DiffuseSpecularMaterial"}
AS_CASES = {"all": (None, False), "subset": (["albedo", ("normal", 2), "roughness"], False), "norm": (None, True),
            "subset_norm": (["albedo", ("normal", 2), "roughness"], True)}
GRAD_LAYOUTS = ("full9", "xy2")
GRAD_SIZE = (19, 29)
NEAR = (32, 64)
NEAR_BAND = 5e-4
GRAD_BAND = 1e-2


def size_key(hw) -> str:
    return "%dx%d" % tuple(hw)


def channels_of(layout: str) -> int:
    return sum(n for _, n in LAYOUTS[layout][1])


def take(packed, layout: str):
    """The channels of the 9-channel input (numpy or torch, [..., 9, H, W]) that `layout` unpacks."""
    c0 = LAYOUTS[layout][0]
    return packed[..., c0:c0 + channels_of(layout), :, :]


def normalized(t):
    """The `is_normalized` form of a [0, 1] input."""
    return t * 2 - 1


def restate_normal_xy(xy: np.ndarray, is_normalized: bool) -> np.ndarray:
    """csrc/packing.hip's NORMAL_XY in numpy float32, every operation rounded on its own, in the kernel's order."""
    f = np.float32
    a = xy.astype(f)
    if is_normalized:
        a = (a * f(0.5) + f(0.5)).astype(f)
    v = (a * f(2) - f(1)).astype(f)
    x, y = v[0], v[1]
    s = ((x * x).astype(f) + (y * y).astype(f)).astype(f)
    z = np.sqrt(np.maximum((f(1) - s).astype(f), f(1e-6))).astype(f)
    n = np.maximum(np.sqrt((s + (z * z).astype(f)).astype(f)).astype(f), f(1e-12))
    return np.stack([(x / n).astype(f), (y / n).astype(f), (z / n).astype(f)])


def _inputs():
    g = torch.Generator().manual_seed(20261018)

    def q(*shape):
        return torch.randint(0, 256, shape, generator=g).to(torch.float32) / 255.0
    z = {}
    for hw in SIZES:
        t = q(9, *hw)
        if hw == (1, 1):
            t[3:5, 0, 0] = torch.tensor([200.0, 90.0]) / 255.0          # a pair inside the circle: z comes from the square root
        z["in__" + size_key(hw)] = t
    # near the unit circle, both sides of the clamp (1 - s >= 1e-6 passes): s = 1 + d, |d| < NEAR_BAND
    n = NEAR[0] * NEAR[1]
    ang = torch.rand(n, generator=g, dtype=torch.float64) * (2 * np.pi)
    d = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * NEAR_BAND
    d[:64] = torch.linspace(-3e-6, 1e-6, 64, dtype=torch.float64)       # a run across the clamp's bound itself
    r = torch.sqrt(1 + d)
    v = torch.stack([r * torch.cos(ang), r * torch.sin(ang)])
    z["nc_in"] = (v * 0.5 + 0.5).to(torch.float32).reshape(2, *NEAR)
    # gradient inputs: quantised, every pair at least GRAD_BAND from the circle
    for layout in GRAD_LAYOUTS:
        t = q(channels_of(layout), *GRAD_SIZE)
        c = [i for i, (name, k) in enumerate(LAYOUTS[layout][1]) if name == "normal"][0]
        c = sum(k for _, k in LAYOUTS[layout][1][:c])
        xy = t[c:c + 2].double() * 2 - 1
        bad = (1 - (xy ** 2).sum(0)).abs() < GRAD_BAND
        t[c, bad], t[c + 1, bad] = 140.0 / 255.0, 100.0 / 255.0
        s = ((t[c:c + 2].double() * 2 - 1) ** 2).sum(0)
        assert ((1 - s).abs() >= GRAD_BAND).all() and (s > 1).any() and (s < 1).any()
        z["g_in__" + layout] = t
        for name, k in LAYOUTS[layout][1]:
            z["g_w__%s__%s" % (layout, name)] = q(3 if (name, k) == ("normal", 2) else k, *GRAD_SIZE) * 2 - 1
    return z


def generate(out_dir: str) -> str:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import import_reference
    import_reference()
    import pypbr.materials as M

    torch.set_num_threads(THREADS)
    z = _inputs()
    worst = 0.0
    for hw in SIZES:
        packed = z["in__" + size_key(hw)]
        for layout, (_, names) in LAYOUTS.items():
            for mode, isn in (("u", False), ("n", True)):
                src = take(normalized(packed) if isn else packed, layout).clone()
                for cls, cls_name in CLASSES.items():
                    m = getattr(M, cls_name).from_tensor(src, names=names, is_normalized=isn)
                    assert type(m).__name__ == cls_name and list(m._maps.keys()) == [n for n, _ in names]
                    for name, k in names:
                        out = m._maps[name]
                        z["ft__%s__%s__%s__%s__%s" % (cls, layout, mode, size_key(hw), name)] = out
                        if (name, k) == ("normal", 2):
                            c = sum(kk for _, kk in names[:[n for n, _ in names].index("normal")])
                            worst = max(worst, float(np.abs(restate_normal_xy(src[c:c + 2].numpy(), isn) - out.numpy()).max()))
        m = M.BasecolorMetallicMaterial.from_tensor(take(packed, "full9").clone(), names=LAYOUTS["full9"][1])
        for case, (names, normalize) in AS_CASES.items():
            z["at__%s__%s" % (size_key(hw), case)] = m.as_tensor(names=names, normalize=normalize)
    for mode, isn in (("u", False), ("n", True)):
        src = normalized(z["nc_in"]) if isn else z["nc_in"]
        out = M.BasecolorMetallicMaterial.from_tensor(src.clone(), names=[("normal", 2)], is_normalized=isn)._maps["normal"]
        z["nc_out__" + mode] = out
        worst = max(worst, float(np.abs(restate_normal_xy(src.numpy(), isn) - out.numpy()).max()))
    assert worst <= 1e-6, "the fp32 restatement of packing.hip's order is %.3e from upstream" % worst
    s = ((z["nc_in"].double() * 2 - 1) ** 2).sum(0)
    assert ((1 - s).abs() < 1.01 * NEAR_BAND).all() and (1 - s < 1e-6).any() and (1 - s >= 1e-6).any()

    envelope = 0.0
    for layout in GRAD_LAYOUTS:
        names = LAYOUTS[layout][1]
        for mode, isn in (("u", False), ("n", True)):
            base = normalized(z["g_in__" + layout]) if isn else z["g_in__" + layout]
            grads = {}
            for dtype in (torch.float64, torch.float32):
                t = base.to(dtype).clone().requires_grad_()
                m = M.BasecolorMetallicMaterial.from_tensor(t, names=names, is_normalized=isn)
                sum((z["g_w__%s__%s" % (layout, name)].to(dtype) * m._maps[name]).sum() for name, _ in names).backward()
                grads[dtype] = t.grad.detach()
            z["g64__%s__%s" % (layout, mode)], z["g32__%s__%s" % (layout, mode)] = grads[torch.float64], grads[torch.float32]
            g64 = grads[torch.float64]
            envelope = max(envelope, float(((grads[torch.float32].double() - g64).abs() / g64.abs().clamp_min(1.0)).max()))

    arrays = {k: np.ascontiguousarray(v.detach().numpy()) for k, v in z.items()}
    for k, v in arrays.items():
        if not k.startswith("g64__"):
            arrays[k] = v.astype(np.float32)
    arrays["meta_grad_envelope"] = np.array([envelope], dtype=np.float64)
    arrays["meta_restatement"] = np.array([worst], dtype=np.float64)
    arrays["meta_torch"] = np.frombuffer(torch.__version__.encode().ljust(32, b"\0"), dtype=np.uint8).astype(np.float32)
    arrays["meta_threads"] = np.array([torch.get_num_threads()], dtype=np.float32)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "packing.npz")
    np.savez_compressed(path, **arrays)
    return path


def meta(z) -> tuple:
    """(torch version, ATen threads) the file was generated with."""
    return bytes(z["meta_torch"].astype(np.uint8)).rstrip(b"\0").decode(), int(z["meta_threads"][0])


if __name__ == "__main__":
    p = generate(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
    zz = np.load(p)
    print("%s: %d bytes, %d arrays, restatement %.3e, gradient envelope %.3e"
          % (p, os.path.getsize(p), len(zz.files), float(zz["meta_restatement"][0]), float(zz["meta_grad_envelope"][0])))
