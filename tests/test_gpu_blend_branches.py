"""Fused-blend gradients where clamps, sRGB knees and back faces decide: cook_torrance_blend_backward_kernel and blend_backward_sink
(ct_blend_backward.hpp), the tiled walk that feeds the same sink (ct_repeat_backward.hpp), and the unfused pieces they replace
(pbr_blend_maps_backward, the decode-normal backward, the render backward, through functional._blend_then_render_with_grad).

Inputs: oracle/branch_cases.py in blend mode -- two materials and a mask whose BLEND is one of the render fixture's cases: normals blended out
to +-80 degrees from two normals 5 to 12 degrees apart and stored at different lengths, masks that hold 0 and 1, colours blended to below 0,
above 1 and under the knees, and flat variants whose blended normal map is decoded again (also onto back faces).
tests/test_blend_branches_host.py holds every case to its populations on the CPU.
Ground truth: float64 autograd of sum(out * W) through blend_oracle.blend_materials and the pinned ATen render oracle.  The rules are
_check_maps of test_gpu_gradient_branches, for both materials' maps and the mask: finite everywhere (the `degenerate` texels included: the
oracle's own float32 gradients are finite there, the host test asserts it), on decided pixels |g - g64| <= BAND (1 + |g64|), exactly 0
on decided back-lit pixels, decided share at least 95 %; and exactly 0 for the material whose weight is 0.  The blended rendering is
held to 1e-5 on ALL pixels, the bound of test_gpu_blend_backward.  No tolerance here is new."""
import ctypes
import functools

import pytest
import torch

import branch_cases as BC
from test_gpu_gradient_branches import _check_maps

pytestmark = pytest.mark.gpu

VARIANTS = BC.all_blend_variants()
IDS = [BC.variant_id(n, kw) for n, kw in VARIANTS]
KW = {BC.variant_id(n, kw): (n, kw) for n, kw in VARIANTS}
ENTRIES = list(BC.BLEND_ENTRY_CONFIGS)
FORWARD_BOUND = 1e-5
FUSED = "_FusedBlendFnBackward"


# the degenerate class (two 2 x 4 blocks, at most 2 % of the texels) exists on the untiled shapes only
RUNS = [pytest.param(vid, entry, id="%s-%s" % (vid, entry)) for vid in IDS for entry in ENTRIES
        if not (KW[vid][1].get("degenerate") and BC.BLEND_ENTRY_CONFIGS[entry][4] != 1)]


@functools.lru_cache(maxsize=None)
def _case(entry, vid):
    """One (variant, entry): built once, its float64 reference computed once (BC.reference caches on the case), never written into."""
    name, kw = KW[vid]
    return BC.build_blend_for(entry, name, kw)


def _naming(case, names):
    """The same case (and its cached reference and decisions), naming only `names` of its gradients."""
    view = case.replace()
    view._cache = case.__dict__.setdefault("_cache", {})
    view.map_names = lambda: list(names)
    return view


def _call_kwargs(case):
    one = case.n_lights == 1
    return dict(view_dir=case.view.float(), light=(case.lights[0] if one else case.lights).float(),
                light_intensity=(case.intensities[0] if one else case.intensities).float(), **case.product_kwargs())


def _leaves(cases):
    """(material 1, material 2, mask) on the device; several cases: material 1 as a batch, material 2 and the mask shared."""
    if len(cases) == 1:
        d1 = {n: t.float().cuda().requires_grad_(True) for n, t in cases[0].first.items()}
    else:
        d1 = {n: torch.stack([c.first[n] for c in cases]).float().cuda().requires_grad_(True) for n in cases[0].first}
    d2 = {n: t.float().cuda().requires_grad_(True) for n, t in cases[0].second.items()}
    return d1, d2, cases[0].mask.float().cuda().requires_grad_(True)


def _render(cases, pieces=False, rows=None, weight=None, **extra):
    """sum(out * W) through functional.cook_torrance(blend=...) (or through the unfused pieces) and its backward.
    -> (out, gradients named like branch_cases.gradients, the autograd node's name)."""
    from pypbr_amd import functional as F
    d1, d2, dm = _leaves(cases)
    if rows is not None:
        cut = lambda t: t.detach()[..., rows[0]:rows[1], :].clone().requires_grad_(True)
        d1, d2, dm = {n: cut(t) for n, t in d1.items()}, {n: cut(t) for n, t in d2.items()}, cut(dm)
    first = [d1.get(n) for n in BC.MAP_NAMES]
    second = tuple(d2.get(n) for n in BC.MAP_NAMES) + (dm,)
    kw = dict(_call_kwargs(cases[0]), **extra)
    out = F._blend_then_render_with_grad(*first, blend=second, **kw) if pieces else F.cook_torrance(*first, blend=second, **kw)
    if weight is None:
        weight = cases[0].weight if len(cases) == 1 else torch.stack([c.weight for c in cases])
    (out * weight.float().cuda()).sum().backward()
    got = {"%d.%s" % (i, n): t.grad.cpu() for i, m in ((1, d1), (2, d2)) for n, t in m.items()}
    got["mask"] = dm.grad.cpu()
    return out.detach().cpu(), got, type(out.grad_fn).__name__


def _check_forward(case, out, tag):
    err = (out.double() - BC.reference(case)["out"]).abs()
    print("%s forward: worst error / 1e-5 %.3f" % (tag, float(err.max()) / FORWARD_BOUND))
    assert float(err.max()) <= FORWARD_BOUND, (tag, "forward", float(err.max()), torch.nonzero(err > FORWARD_BOUND)[:4].tolist())


def _check_unused_material(case, got, tag):
    """Where the mask is 0 material 1 has weight 0, where it is 1 material 2 has: their gradients are exactly 0 there."""
    for name in case.map_names():
        if name != "mask":
            unused = case.mask[0] == (0.0 if name[0] == "1" else 1.0)
            assert float(unused.double().mean()) >= 0.10, (tag, name)
            g = got[name][:, unused]
            assert bool((g == 0).all()), (tag, name, "gradient of the material with weight 0", float(g.abs().max()))


def _check(case, got, tag):
    _check_maps(case, got, BC.reference(case), tag)
    _check_unused_material(case, got, tag)


def _serves(case):
    """pbr_blend_backward_serves for the plan of this case's call."""
    from pypbr_amd import _native as N
    from pypbr_amd import functional as F
    d1, d2, dm = _leaves([case])
    det = lambda t: None if t is None else t.detach()
    plan = F.plan_cook_torrance(*[det(d1.get(n)) for n in BC.MAP_NAMES], blend=tuple(det(d2.get(n)) for n in BC.MAP_NAMES) + (dm.detach(),),
                                **_call_kwargs(case))
    return plan.desc.map_height, N.lib().pbr_blend_backward_serves(ctypes.byref(plan.desc))


@pytest.mark.parametrize("vid,entry", RUNS)
def test_blend_gradients_on_every_branch(vid, entry):
    """Both materials' maps and the mask through every entry of the blend's chain rule: two pixels per lane (24x40) and one (23x37, and once
    more under the public tuning={"max_vec": 1}), three lights, a 12x16 map tiled 2x2 (the fused tiled backward: it must serve), and the
    unfused pieces called directly."""
    case = _case(entry, vid)
    tag = "%s %s" % (vid, entry)
    pieces = entry == "blend-pieces"
    if case.tile != 1:
        assert _serves(case) == (case.albedo.shape[1], 1), tag
    for extra in ([{}, dict(tuning={"max_vec": 1})] if entry == "blend-one-pixel" else [{}]):
        out, got, node = _render([case], pieces=pieces, **extra)
        assert pieces or node == FUSED, (tag, node)          # the fused kernels, not the fallback
        label = tag + (", max_vec 1" if extra else "")
        _check_forward(case, out, label)
        _check(case, got, label)


@pytest.mark.parametrize("entry,name,kw", BC.BLEND_BATCH_CASES, ids=[e + "-" + BC.variant_id(n, kw) for e, n, kw in BC.BLEND_BATCH_CASES])
def test_batch_of_two_first_materials_against_one_second_material_and_mask(entry, name, kw):
    """B = 2 first materials (seeds 0 and 2), one second material, one mask: material 1's gradients per material, the shared ones own the sum."""
    cases = BC.build_blend_batch(entry, name, kw)
    out, got, node = _render(cases)
    assert node == FUSED and out.shape[0] == 2
    shared = {n: sum(BC.reference(c)[n] for c in cases) for n in cases[0].map_names() if n[0] != "1"}
    both = BC.decided(cases[0]) & BC.decided(cases[1])
    assert float(both.double().mean()) >= 0.90
    for b, case in enumerate(cases):
        tag = "%s %s material %d of a batch" % (BC.variant_id(name, kw), entry, b)
        _check_forward(case, out[b], tag)
        first = _naming(case, [n for n in case.map_names() if n[0] == "1"])          # the shared ones own the sum: checked below
        _check(first, {n: got[n][b] for n in first.map_names()}, tag)
    for n, want in shared.items():
        g = got[n].reshape(want.shape)
        assert bool(torch.isfinite(g).all()), n
        err, band = (g.double() - want).abs(), BC.BAND * (1 + want.abs())
        print("%s %s shared %-11s worst error / band %.3f" % (BC.variant_id(name, kw), entry, n, float((err / band)[:, both].max())))
        assert not bool(((err > band) & both).any()), (n, float((err / band)[:, both].max()))
        dark = BC.backlit(cases[0]) & BC.backlit(cases[1]) & both
        assert bool((g[:, dark] == 0).all()), n


@pytest.mark.parametrize("vid", ["backlit", "backlit-flat=True"])
def test_a_row_band_with_given_flags_equals_the_rows_of_the_whole_map(vid):
    """Rows [6, 19) of the 24x40 point-light case with the whole map's flag given (blend_flags): bit-equal to the whole map's rows, for a
    signed blended normal map and for a flat one whose band crosses the back-lit columns."""
    case = _case("blend-pairs-point", vid)
    y0, y1 = 6, 19
    whole_out, whole, node = _render([case])
    flags = torch.tensor([0 if case.flat else 1], dtype=torch.int32, device="cuda")
    out, band, band_node = _render([case], rows=(y0, y1), weight=case.weight[:, y0:y1], y_offset=y0, height_total=case.albedo.shape[1], blend_flags=flags)
    assert node == FUSED and band_node == FUSED
    assert float((BC.backlit(case) & BC.decided(case))[y0:y1].double().mean()) >= 0.10
    assert torch.equal(out, whole_out[:, y0:y1])
    for n in case.map_names():
        assert torch.equal(band[n], whole[n][:, y0:y1]), (vid, n)


@pytest.mark.parametrize("vid", IDS)
def test_fused_kernel_against_the_unfused_pieces(vid):
    """The same device, the same inputs, two implementations: what separates a wrong blend chain rule from a wrong fixture when something
    above fails.  Tolerance: test_fused_blend_backward_equals_the_unfused_differentiable_pieces'."""
    case = _case("blend-pieces", vid)
    fo, fused, node = _render([case])
    po, pieces, _ = _render([case], pieces=True)
    assert node == FUSED
    assert float((fo - po).abs().max()) <= 2e-6
    keep = ~case.degenerate                      # a blend of length 0 divides by the floor under its norm: 1e12 times rounding noise on either side
    for n in case.map_names():
        a, b = fused[n][:, keep], pieces[n][:, keep]
        d, tol = float((a - b).abs().max()), 2e-5 * (1 + float(b.abs().max()))
        print("%s %-11s fused - pieces %.3e, tolerance %.3e" % (vid, n, d, tol))
        assert d <= tol, (vid, n, d, tol)
