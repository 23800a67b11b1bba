"""The stand-alone map ops (csrc/map_ops.hip) and the sigmoid mask (csrc/blend.hip) on BUILT inputs: values and gradients where the
reference's clamps, knees and thresholds decide.

The inputs are oracle/map_op_cases.py's (held on the CPU by tests/test_map_op_cases_host.py): every site a known distance from every
threshold the reference compares, every named branch on at least 10 % of the elements, at least 95 % of the sites decided.  Every case runs
through every layout of map_op_cases.LAYOUTS by the C entry points, inside guard bands (tests/test_gpu_write_guards.Guards):

    quads       a length divisible by 4, every buffer 16-byte aligned: the 4-element lanes
    tail-1/2/3  3 x 23 x 37 and its two neighbours: lengths 4 k + 1, 4 k + 2, 4 k + 3 -- the scalar tail behind the quads (per-pixel ops
                and the mask: 851, 874, 897 sites per plane, their one-element forms)
    unaligned   every buffer one element off a 16-byte boundary inside a larger allocation: every pointer fails the alignment test
    tiny        1, 3 and 5 sites

in float32 and float16 storage wherever the C entry takes a dtype, and at the `quads` and `tail-1` shapes through pypbr_amd.functional,
the torch.ops.pbr_hip bindings and the material API (to_basecolor_metallic_material, to_diffuse_specular_material, to_linear / to_srgb,
blending.sigmoid_mask, a normal assigned in a constructor), the conversions also as a batch of 2.

Forward: on decided sites fp32 results are within 2e-6 of float64; fp16 results equal, bit for bit, the fp32 kernel's result on the same
(fp16-exact) inputs rounded once to fp16; mask and metallic results are exactly 0 or 1 where float64 is.
Gradients: finite on ALL sites; on decided sites |g - g64| <= 2e-5 (1 + |g64|), fp16 storage adds 1e-3 (1e-3 + |g64|) (the rule of
tests/test_gpu_gradient_branches.py); where float64 autograd gives exactly 0 on a decided site -- outside [0, 1], `dead`, `q_below_0`,
`q_above_1`, `basecolor_clamped`, the specular gradient off the `metal` branch when only the basecolor is used -- the kernel gives exactly
0; a kept 3-channel normal map passes the gradient through bit for bit.
The sigmoid mask only: its backward reads the STORED float32 mask and forms sg (1 - sg); one ulp of a mask near 1 is 2^-24 and moves
sg (1 - sg) / (width + 1e-6) by that much times |G| / (width + 1e-6), so its bound has the term 2^-23 |G| / (width + 1e-6) added
(map_op_cases.storage_term).  That term is DERIVED from the storage format, not measured.
No other bound is widened: no op needed the envelope form.  Every test prints its worst error / band per layout (run with -s); measured
on an MI355X the highest are 0.68 (to_basecolor_metallic, sRGB diffuse, fp32), 0.47 (every op on fp16 storage: the rounding of the stored
gradient), 0.12 (2-channel decode; the mask at width 0.001) and under 0.03 for everything else."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import branch_cases as BC
import map_op_cases as MC
import torch_oracle as O
from test_gpu_write_guards import G, Guards, P, _lib, _stream

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16}
VARIANTS = MC.all_variants()
IDS = [MC.variant_id(op, kw) for op, kw in VARIANTS]
API_LAYOUTS = ("quads", "tail-1")          # the shapes the wrappers can express: whole [C,h,w] maps in allocations of their own
IN_NAMES = {"to_basecolor_metallic": ("diffuse", "specular"), "to_diffuse_specular": ("albedo", "metallic"), "srgb_to_linear": ("x",),
            "linear_to_srgb": ("x",), "decode_normal": ("normal",), "sigmoid_mask": ("prop1", "prop2")}
OUT_NAMES = {"to_basecolor_metallic": ("basecolor", "metallic"), "to_diffuse_specular": ("diffuse", "specular")}


@functools.lru_cache(maxsize=None)
def _case_cached(op, kw_items, layout, seed):
    return MC.build_for(op, dict(kw_items), layout, seed=seed)


def _case(op, kw, layout, seed=0):
    """One case object per (op, variant, layout, seed): its float64 reference is computed once and shared by every test."""
    return _case_cached(op, tuple(sorted(kw.items())), layout, seed)


def _dtypes(op):
    return ("f32", "f16") if op in MC.TAKES_DTYPE else ("f32",)


# ------------------------------------------------------------------------------------------------ the assertions
def _check(case, out, grads, dtype, tag, use=None):
    """`out` / `grads`: name -> device tensor of any shape holding the flat list.  -> worst gradient error / band on decided sites."""
    ref = MC.reference(case) if use is None else MC.gradients(case, use=use)
    keep = MC.decided(case)
    share = float(keep.double().mean())
    assert share >= 0.95 if case.n > 5 else share == 1.0, (tag, share)
    for name, got in out.items():
        want = ref["out"][name]
        got = got.detach().cpu().double().reshape(want.shape)
        if dtype == torch.float32:
            err = (got - want).abs()[..., keep]
            assert float(err.max()) <= 2e-6, (tag, name, "forward", float(err.max()))
        if name == "metallic" or case.op == "sigmoid_mask":
            for end in (0.0, 1.0):
                sel = (want == end) & keep
                assert bool((got[sel] == end).all()), (tag, name, "exactly %g in float64" % end, int((got[sel] != end).sum()))
    worst = 0.0
    for name, got in grads.items():
        g64 = ref[name]
        got = got.detach().cpu().double().reshape(g64.shape)
        assert bool(torch.isfinite(got).all()), (tag, name, "non-finite gradient")
        band = MC.band(case, g64) + (1e-3 * (1e-3 + g64.abs()) if dtype == torch.float16 else 0.0)
        ratio = ((got - g64).abs() / band)[..., keep]
        worst = max(worst, float(ratio.max()))
        assert worst <= 1.0, (tag, name, "gradient error / band", worst)
        zero = (g64 == 0) & keep
        assert bool((got[zero] == 0).all()), (tag, name, "a selected-away branch leaks", int((got[zero] != 0).sum()), float(got[zero].abs().max()))
    return worst


# ------------------------------------------------------------------------------------------------ the C entry points, guarded
def _c_route(case, dtype, off, use=None, want=None, zeros_for_absent=False):
    """Forward and backward of the case through the C entry points, every buffer `off` elements off a 16-byte boundary inside guard bands.
    use: the outputs whose upstream gradient is passed (the others NULL, or all-zero buffers with zeros_for_absent); want: the gradients
    asked for (the others NULL).  -> (out, grads): name -> device tensor."""
    N, lib = _lib()
    st = _stream()
    code = N.F16 if dtype == torch.float16 else N.F32
    op, kw, n = case.op, case.variant, case.n
    gd = Guards(G + off)
    x = {k: gd.input(v.to(dtype)) for k, v in case.inputs.items()}
    outs_all = tuple(case.weights)
    use = outs_all if use is None else use
    want = IN_NAMES[op] if want is None else want
    if op == "decode_normal" and dtype != torch.float32:
        want = ()                                      # the decode's backward is float32 only
    up = {k: (gd.input(case.weights[k].to(dtype)) if k in use else (gd.input(torch.zeros_like(case.weights[k]).to(dtype)) if zeros_for_absent else None))
          for k in outs_all}
    out = {k: gd.output(tuple(case.weights[k].shape), dtype) for k in outs_all}
    g = {k: (gd.output(tuple(case.inputs[k].shape), dtype) if k in want else None) for k in IN_NAMES[op]}
    tag = (MC.variant_id(op, kw), n, off, str(dtype), use, want)
    if op == "to_basecolor_metallic":
        srgb = int(kw["albedo_is_srgb"])
        N.check(lib.pbr_specular_to_metallic(P(x["diffuse"]), P(x["specular"]), P(out["basecolor"]), P(out["metallic"]), n, srgb, code, st))
        N.check(lib.pbr_specular_to_metallic_backward(P(x["diffuse"]), P(x["specular"]), P(up["basecolor"]), P(up["metallic"]), P(g["diffuse"]),
                                                      P(g["specular"]), n, srgb, code, st))
    elif op == "to_diffuse_specular":
        srgb = int(kw["albedo_is_srgb"])
        N.check(lib.pbr_metallic_to_specular(P(x["albedo"]), P(x["metallic"]), P(out["diffuse"]), P(out["specular"]), 1, n, srgb, code, st))
        N.check(lib.pbr_metallic_to_specular_backward(P(x["albedo"]), P(x["metallic"]), P(up["diffuse"]), P(up["specular"]), P(g["albedo"]),
                                                      P(g["metallic"]), 1, n, srgb, code, st))
    elif op in ("srgb_to_linear", "linear_to_srgb"):
        fwd, bwd = ((lib.pbr_srgb_to_linear, lib.pbr_srgb_to_linear_backward) if op == "srgb_to_linear" else
                    (lib.pbr_linear_to_srgb, lib.pbr_linear_to_srgb_backward))
        N.check(fwd(P(x["x"]), P(out["out"]), n, code, st))
        N.check(bwd(P(x["x"]), P(up["out"]), P(g["x"]), n, code, st))
    elif op == "decode_normal":
        flag = gd.workspace(4)
        N.check(lib.pbr_decode_normal(P(x["normal"]), P(out["out"]), kw["channels"], n, code, P(flag), st))
        if want:
            N.check(lib.pbr_decode_normal_backward(P(x["normal"]), P(up["out"]), P(g["normal"]), kw["channels"], n, P(flag), st))
    else:
        N.check(lib.pbr_blend_sigmoid_mask(P(x["prop1"]), P(x["prop2"]), P(out["out"]), n, kw["shift"], kw["blend_width"], st))
        torch.cuda.synchronize()
        stored = gd.input(out["out"].clone())          # the backward reads the stored mask
        N.check(lib.pbr_blend_sigmoid_mask_backward(P(stored), P(up["out"]), P(g["prop1"]), P(g["prop2"]), n, kw["blend_width"], st))
    gd.check(tag)
    return out, {k: v for k, v in g.items() if v is not None}


@pytest.mark.parametrize("op,kw", VARIANTS, ids=IDS)
def test_every_layout_through_the_c_entry_points(op, kw):
    for dt in _dtypes(op) + (("f16",) if op == "decode_normal" else ()):          # the decode's forward takes fp16 maps too
        dtype = DTYPES[dt]
        line = []
        for layout, (_, off) in MC.LAYOUTS.items():
            case = _case(op, kw, layout)
            tag = (MC.variant_id(op, kw), layout, dt)
            out, grads = _c_route(case, dtype, off)
            if dtype == torch.float16:          # storage only: the fp32 kernel's result on the same values, rounded once
                out32, _ = _c_route(case, torch.float32, off)
                for name in out:
                    assert torch.equal(out[name], out32[name].half()), (tag, name, "fp16 forward is not the fp32 result rounded once")
            worst = _check(case, out, grads, dtype, tag)
            line.append("%s %.3f" % (layout, worst) if grads else "%s forward only" % layout)
            if op == "decode_normal" and kw.get("kept") and grads:
                assert torch.equal(grads["normal"].cpu().double(), case.weights["out"]), (tag, "a kept map passes the gradient through")
                assert torch.equal(out["out"].cpu().double(), case.inputs["normal"]), (tag, "a kept map is kept")
        print("%-44s %s worst error / band: %s" % (MC.variant_id(op, kw), dt, "  ".join(line)))


# ------------------------------------------------------------------------------------------------ functional, torch op, material API
def _call(op, kw, binding, x):
    """The op through one of its public bindings on device tensors shaped as maps.  -> dict output name -> tensor."""
    from pypbr_amd import blending, functional as F
    from pypbr_amd.materials import BasecolorMetallicMaterial, DiffuseSpecularMaterial, MaterialBase
    dev = torch.device("cuda", torch.cuda.current_device())
    ops = torch.ops.pbr_hip
    if op == "to_basecolor_metallic":
        srgb = kw["albedo_is_srgb"]
        if binding == "material":
            back = DiffuseSpecularMaterial(albedo=x["diffuse"], albedo_is_srgb=srgb, specular=x["specular"], specular_is_srgb=False,
                                           device=dev).to_basecolor_metallic_material()
            return dict(basecolor=back._maps["albedo"], metallic=back._maps["metallic"])
        fn = F.diffuse_specular_to_basecolor_metallic if binding == "functional" else ops.diffuse_specular_to_basecolor_metallic
        return dict(zip(OUT_NAMES[op], fn(x["diffuse"], x["specular"], srgb)))
    if op == "to_diffuse_specular":
        srgb = kw["albedo_is_srgb"]
        if binding == "material":
            conv = BasecolorMetallicMaterial(albedo=x["albedo"], albedo_is_srgb=srgb, metallic=x["metallic"], device=dev).to_diffuse_specular_material()
            return dict(diffuse=conv._maps["albedo"], specular=conv._maps["specular"])
        fn = F.metallic_to_diffuse_specular if binding == "functional" else ops.metallic_to_diffuse_specular
        return dict(zip(OUT_NAMES[op], fn(x["albedo"], x["metallic"], srgb)))
    if op in ("srgb_to_linear", "linear_to_srgb"):
        if binding == "material":
            mat = MaterialBase(albedo=x["x"], albedo_is_srgb=op == "srgb_to_linear", device=dev)
            return dict(out=(mat.to_linear() if op == "srgb_to_linear" else mat.to_srgb())._maps["albedo"])
        return dict(out=getattr(F if binding == "functional" else ops, op)(x["x"]))
    if op == "decode_normal":
        if binding == "material":
            return dict(out=BasecolorMetallicMaterial(normal=x["normal"], device=dev)._maps["normal"])
        return dict(out=F.decode_normal(x["normal"]))
    return dict(out=blending.sigmoid_mask(x["prop1"], x["prop2"], kw["blend_width"], kw["shift"]))


BINDINGS = {"to_basecolor_metallic": ("functional", "torch_op", "material"), "to_diffuse_specular": ("functional", "torch_op", "material"),
            "srgb_to_linear": ("functional", "torch_op", "material"), "linear_to_srgb": ("functional", "torch_op", "material"),
            "decode_normal": ("functional", "material"), "sigmoid_mask": ("functional",)}


def _api_route(cases, layout, dtype, binding, use=None):
    """The cases (one, or the materials of a batch) as [C,h,w] / [B,C,h,w] maps through a public binding; gradients by autograd of
    sum(out * weight) over the outputs in `use`.  -> per case (out, grads)."""
    op, kw = cases[0].op, cases[0].variant
    (h, w), _ = MC.LAYOUTS[layout]
    maps = lambda t: t.reshape(-1, h, w)
    stack = lambda ts: (torch.stack(ts) if len(ts) > 1 else ts[0])
    x = {k: stack([maps(c.inputs[k]) for c in cases]).to(dtype).cuda().requires_grad_(True) for k in IN_NAMES[op]}
    out = _call(op, kw, binding, x)
    wts = {k: stack([maps(c.weights[k]) for c in cases]).cuda() for k in out}
    for name, t in out.items():
        assert t.dtype == dtype and t.requires_grad, (op, binding, name)
    sum((out[k].float() * wts[k].float()).sum() for k in (tuple(out) if use is None else use)).backward()
    pick = (lambda t, b: t[b]) if len(cases) > 1 else (lambda t, b: t)
    res = []
    for b in range(len(cases)):
        res.append(({k: pick(v, b) for k, v in out.items()}, {k: pick(v.grad, b) for k, v in x.items()}))
        for k, v in x.items():
            assert v.grad is not None and v.grad.dtype == dtype, (op, binding, k)
    return res


@pytest.mark.parametrize("op,kw", VARIANTS, ids=IDS)
def test_public_bindings_on_whole_maps(op, kw):
    from pypbr_amd import torch_ops
    assert torch_ops.available()
    for binding in BINDINGS[op]:
        for dt in (_dtypes(op) if binding != "material" else ("f32",)):
            line = []
            for layout in API_LAYOUTS:
                case = _case(op, kw, layout)
                tag = (MC.variant_id(op, kw), layout, dt, binding)
                (out, grads), = _api_route([case], layout, DTYPES[dt], binding)
                line.append("%s %.3f" % (layout, _check(case, out, grads, DTYPES[dt], tag)))
            print("%-44s %s %-10s worst error / band: %s" % (MC.variant_id(op, kw), dt, binding, "  ".join(line)))


@pytest.mark.parametrize("op", ["to_basecolor_metallic", "to_diffuse_specular"])
@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_conversions_as_a_batch_of_two(op, srgb, dt):
    kw = dict(albedo_is_srgb=srgb)
    for layout in API_LAYOUTS:
        cases = [_case(op, kw, layout, seed) for seed in (0, 1)]
        for binding in ("functional", "torch_op"):
            for b, (out, grads) in enumerate(_api_route(cases, layout, DTYPES[dt], binding)):
                worst = _check(cases[b], out, grads, DTYPES[dt], (op, srgb, dt, layout, binding, "material", b))
                print("%-44s %s %-10s %-7s material %d worst error / band %.3f" % (MC.variant_id(op, kw), dt, binding, layout, b, worst))


# ------------------------------------------------------------------------------------------------ optional arguments of the conversion backwards
@pytest.mark.parametrize("op", ["to_basecolor_metallic", "to_diffuse_specular"])
@pytest.mark.parametrize("srgb", [True, False])
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_absent_upstreams_and_unwanted_results_of_the_conversion_backwards(op, srgb, dt):
    """Each upstream gradient absent (NULL) in turn: the results are torch.equal to the call with an all-zero upstream in its place, and
    held to float64 autograd of the one output that is used (so the specular gradient is exactly 0 off the `metal` branch when only the
    basecolor is used).  Each result unwanted (NULL) in turn: the remaining one is torch.equal to the full call's; guard bands around
    everything."""
    kw, dtype = dict(albedo_is_srgb=srgb), DTYPES[dt]
    for layout in ("quads", "tail-1", "tail-3", "unaligned", "tiny-3"):
        case, off = _case(op, kw, layout), MC.LAYOUTS[layout][1]
        tag = (op, srgb, dt, layout)
        _, full = _c_route(case, dtype, off)
        for used in OUT_NAMES[op]:
            _, got = _c_route(case, dtype, off, use=(used,))
            _, zeroed = _c_route(case, dtype, off, use=(used,), zeros_for_absent=True)
            for name in got:
                assert torch.equal(got[name], zeroed[name]), (tag, "only", used, name)
            worst = _check(case, {}, got, dtype, tag + ("only", used), use=(used,))
            print("%-44s %s %-9s only %-9s used: worst error / band %.3f" % (MC.variant_id(op, kw), dt, layout, used, worst))
        for wanted in IN_NAMES[op]:
            _, got = _c_route(case, dtype, off, want=(wanted,))
            assert tuple(got) == (wanted,) and torch.equal(got[wanted], full[wanted]), (tag, "alone", wanted)


# ------------------------------------------------------------------------------------------------ one chain through the public API
def _chain_inputs(srgb):
    """The conversion case at 3 x 24 x 40 as predicted maps, the render fixture's normals, roughness, light and view, a target image."""
    (h, w), _ = MC.LAYOUTS["quads"]
    conv = _case("to_basecolor_metallic", dict(albedo_is_srgb=srgb), "quads")
    render = BC.build("albedo_range", h, w, light_type="directional", workflow="metallic", albedo_is_srgb=True, return_srgb=True)
    target = BC.render(BC.build("albedo_range", h, w, light_type="directional", seed=1)).float()
    return conv, render, target, conv.inputs["diffuse"].reshape(3, h, w), conv.inputs["specular"].reshape(3, h, w)


def _chain64(srgb):
    """float64 autograd of the chain of oracle ops.  -> (loss, g_diffuse, g_specular, keep [3,h,w])."""
    conv, render, target, d0, s0 = _chain_inputs(srgb)
    d64, s64 = d0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
    base, met3 = O.diffuse_specular_to_basecolor_metallic(O.srgb_to_linear(d64) if srgb else d64, s64)
    met = met3.mean(dim=0, keepdim=True)
    enc = O.linear_to_srgb(base)
    img = O.cook_torrance(enc, render.normal, render.roughness, met, None, view=render.view, light=render.lights[0], intensity=render.intensities[0],
                          light_type="directional", albedo_is_srgb=True, return_srgb=True)
    loss = TF.mse_loss(img, target.double())
    loss.backward()
    # the render's own rule on the maps it is handed.  A basecolor the conversion clamped to exactly 0.0 or 1.0 (decided there: the same
    # side in every precision) encodes to a clamp end of the decode: stored as that end, it is an exact end as in the fixture's `closed_ends`
    b = base.detach()
    ends = torch.where(b == 1, torch.ones_like(b), torch.where(b == 0, torch.zeros_like(b), enc.detach()))
    chained = render.replace(name="closed_ends", albedo=ends, metallic=met.detach())
    keep = MC.decided(conv).reshape(d0.shape) & BC.threshold_decided(chained).unsqueeze(0)
    return loss.detach(), d64.grad, s64.grad, keep


@pytest.mark.parametrize("srgb", [True, False])
def test_predicted_maps_through_conversion_encode_render_and_loss(srgb):
    """Predicted diffuse and specular maps (the conversion case, 3 x 24 x 40) -> to_basecolor_metallic_material() -> to_srgb() ->
    CookTorranceBRDF -> MSE, against float64 autograd of the same chain of oracle ops.

    ONE STEP MORE THAN THAT CHAIN: the conversion yields a 3-channel metallic map (diffuse.py:147); the reference's renderer broadcasts it
    per channel, this package's renderer takes a 1-channel metallic map only (functional._as_batched raises ValueError on three).  A user
    has to reduce it; the chain here assigns `material.metallic = metallic.mean(0, keepdim=True)` (plain torch on the device, autograd's
    own backward), in the product chain and in the oracle chain alike, so every channel of the conversion's metallic result still carries a
    gradient from the rendering.

    An element counts when the conversion's `decided` holds for it and its pixel is threshold-decided by the render fixture's own rule
    (branch_cases.threshold_decided on the maps the renderer is handed).  The band is relative to the largest |g64| of the map (the loss is
    a mean over all pixels), the bound of test_rendering_loss_through_the_material_conversions."""
    from pypbr_amd.materials import DiffuseSpecularMaterial
    from pypbr_amd.models import CookTorranceBRDF
    conv, render, target, d0, s0 = _chain_inputs(srgb)
    loss64, gd64, gs64, keep = _chain64(srgb)
    dev = torch.device("cuda", torch.cuda.current_device())
    dd, sd = d0.float().cuda().requires_grad_(True), s0.float().cuda().requires_grad_(True)
    mat = DiffuseSpecularMaterial(albedo=dd, albedo_is_srgb=srgb, normal=render.normal.float().cuda(), roughness=render.roughness.float().cuda(),
                                  specular=sd, specular_is_srgb=False, device=dev)
    back = mat.to_basecolor_metallic_material()
    back.to_srgb()
    assert back.albedo_is_srgb and back._maps["metallic"].shape[0] == 3
    back.metallic = back._maps["metallic"].mean(dim=0, keepdim=True)
    img = CookTorranceBRDF("directional")(back, render.view.float(), render.lights[0].float(), render.intensities[0].float())
    loss = TF.mse_loss(img, target.cuda())
    loss.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-6, (loss.item(), loss64.item())
    share = float(keep.double().mean())
    print("chain srgb=%s: %.1f %% of the elements compared" % (srgb, 100 * share))
    assert share >= 0.95, share         # from the oracles alone: 97.3 % (sRGB) and 100 % (linear)
    for name, got, want in (("diffuse", dd.grad, gd64), ("specular", sd.grad, gs64)):
        got = got.cpu().double()
        assert bool(torch.isfinite(got).all()), name
        bound = 2e-5 * (float(want.abs().max()) + 1e-6) + 2e-9
        ratio = (got - want).abs()[keep] / bound
        print("chain srgb=%s %s: worst error / bound %.3f (largest |g64| %.3g)" % (srgb, name, float(ratio.max()), float(want.abs().max())))
        assert float(ratio.max()) <= 1.0, (name, float(ratio.max()))
