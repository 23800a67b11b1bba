"""The map-op fixture (oracle/map_op_cases.py) held to its promises, on the CPU, with the oracles only: this is where the inputs of
tests/test_gpu_map_op_branches.py get fixed.  For every op and variant, at every layout that test runs:

  * at least 95 % of the sites are decided (threshold-decided and well conditioned);
  * every named branch holds at least 10 % of the elements, and at least 5 % of the elements are on it AND decided -- but for the branches
    of the sigmoid mask that a width / shift pair leaves empty by construction (map_op_cases.empty_by_construction), and at the `tiny`
    layouts, whose 1, 3 and 5 sites cannot hold seven branches at 10 % each: there every site must be decided instead;
  * the quantities `decisions` reads rebuild the oracle's outputs to 1e-14;
  * the oracle's own float32 forward is within 2e-6 of its float64 forward on decided sites;
  * the conversion: the plain-C oracle in float32 (c_oracle.specular_to_metallic) takes the same side of every select as float64 on every
    decided element, and live elements keep |den| >= 0.02.

These caps are conditions on the inputs: a case that misses one gets other inputs, never another cap.  Run with -s to see the populations."""
import numpy as np
import pytest
import torch

import c_oracle as C
import map_op_cases as MC

VARIANTS = MC.all_variants()
IDS = [MC.variant_id(op, kw) for op, kw in VARIANTS]


@pytest.mark.parametrize("op,kw", VARIANTS, ids=IDS)
def test_every_case_populates_its_branches_and_stays_decided(op, kw):
    for layout in MC.LAYOUTS:
        case = MC.build_for(op, kw, layout)
        tag = (MC.variant_id(op, kw), layout)
        print("%-10s %s" % (layout, MC.report(case)))
        assert case.n == MC.sites(op, layout), tag
        decided = MC.decided(case)
        share = float(decided.double().mean())
        if layout not in MC.POPULATED_LAYOUTS:
            assert share == 1.0, (tag, share)
            continue
        assert share >= 0.95, (tag, share)
        for name, mask in MC.branches(case).items():
            if name in MC.exempt(case):
                assert not bool(mask.any()), (tag, name, "named empty by construction, but populated")
                continue
            assert float(mask.double().mean()) >= 0.10, (tag, name, float(mask.double().mean()))
            assert float((mask & decided).double().mean()) >= 0.05, (tag, name, float((mask & decided).double().mean()))


@pytest.mark.parametrize("op,kw", VARIANTS, ids=IDS)
def test_the_decisions_are_read_from_the_oracle(op, kw):
    for layout in MC.LAYOUTS:
        case = MC.build_for(op, kw, layout)
        tag = (MC.variant_id(op, kw), layout)
        ref, ref32 = MC.reference(case), MC.forward(case, dtype=torch.float32)
        decided = MC.decided(case)
        for name, want in MC.restated(case).items():
            assert (want - ref["out"][name]).abs().max().item() <= 1e-14, (tag, name)
            err = (ref32[name].double() - ref["out"][name]).abs()
            assert float(err[..., decided].max()) <= 2e-6, (tag, name, float(err[..., decided].max()))
        for name in case.inputs:
            assert bool(torch.isfinite(ref[name]).all()) and bool(torch.isfinite(MC.gradients(case, torch.float32)[name]).all()), (tag, name)


@pytest.mark.parametrize("srgb", [True, False])
def test_the_c_oracle_takes_the_same_side_of_every_select(srgb):
    for layout in MC.LAYOUTS:
        case = MC.build_for("to_basecolor_metallic", dict(albedo_is_srgb=srgb), layout)
        d, s = (case.inputs[k].float().numpy() for k in ("diffuse", "specular"))
        lin = C.srgb_to_linear(d) if srgb else d
        planes = lambda x: np.stack([x, x, x]).reshape(3, 1, -1)          # the C oracle converts three planes of P pixels
        b32, m32 = (torch.from_numpy(x[0, 0]) for x in C.specular_to_metallic(planes(lin), planes(s)))
        out, keep = MC.reference(case)["out"], MC.decided(case)
        b64, m64 = out["basecolor"], out["metallic"]
        for what, got, want in (("metallic is 0", m32 == 0, m64 == 0), ("metallic is 1", m32 == 1, m64 == 1),
                                ("metallic >= 0.95", m32 >= 0.95, m64 >= 0.95), ("basecolor is 0", b32 == 0, b64 == 0),
                                ("basecolor is 1", b32 == 1, b64 == 1)):
            assert torch.equal(got[keep], want[keep]), (srgb, layout, what, int((got != want)[keep].sum()))
        t = MC._s2m_terms(case)
        assert bool((t["den"].abs() >= MC.DEN_FLOOR).all()), (srgb, layout, float(t["den"].abs().min()))


def test_cases_are_deterministic_fp16_exact_and_differ_by_seed():
    for op, kw in VARIANTS:
        a, b, c = (MC.build(op, seed=s, n=851, **kw) for s in (0, 0, 1))
        for name, x in a.inputs.items():
            assert x.dtype == torch.float64 and torch.equal(x, x.half().double()), (op, kw, name)
            assert torch.equal(x, b.inputs[name]), (op, kw, name)
        assert any(not torch.equal(x, c.inputs[name]) for name, x in a.inputs.items() if float(x.std()) > 0), (op, kw)
        for name, w in a.weights.items():
            assert torch.equal(w, b.weights[name]) and 0.25 <= float(w.abs().min()) and float(w.abs().max()) <= 1.0, (op, kw, name)
            assert bool((w > 0).any()) and bool((w < 0).any()), (op, kw, name)


def test_what_the_variants_promise():
    """Exact ends are stored where the fixture says so; the kept normal map has its one negative value; the mask's empty branches are the
    ones reasoned out in the fixture (shift -0.5 at width 0.001 has no transition)."""
    for op, kw in VARIANTS:
        case = MC.build(op, **kw)
        if case.exact_ends:
            x = case.inputs["diffuse" if op == "to_basecolor_metallic" else ("albedo" if op == "to_diffuse_specular" else "x")]
            assert bool((x == 0).any()) and bool((x == 1).any()), (op, kw)
        if op == "decode_normal" and kw["channels"] == 3:
            nm = case.inputs["normal"]
            assert int((nm < 0).sum()) == (1 if kw["kept"] else 0) and (not kw["kept"] or float(nm[0, 0]) == MC.KEPT_VALUE), kw
            if kw["kept"]:          # the oracle keeps the map and passes the gradient through: bit for bit the upstream weight
                ref = MC.reference(case)
                assert torch.equal(ref["out"]["out"], nm) and torch.equal(ref["normal"], case.weights["out"])
    assert "transition" in MC.empty_by_construction(0.001, -0.5) and MC.empty_by_construction(0.005, 0.0) == ()
    assert MC.empty_by_construction(0.5, 0.0) == ("saturated_high", "saturated_low")


def test_the_rule_on_arbitrary_inputs_is_the_rule_of_the_cases():
    """decided_to_basecolor_metallic on a built case's own inputs is that case's `decided`."""
    for srgb in (True, False):
        case = MC.build("to_basecolor_metallic", albedo_is_srgb=srgb, n=2553)
        got = MC.decided_to_basecolor_metallic(case.inputs["diffuse"].reshape(3, 23, 37), case.inputs["specular"].reshape(3, 23, 37), srgb,
                                               case.weights["basecolor"], case.weights["metallic"])
        assert got.shape == (3, 23, 37) and torch.equal(got.reshape(-1), MC.decided(case))
        g = torch.Generator().manual_seed(1)          # random maps: elements with |den| < 0.02 are live and left out
        d, s = torch.rand(2000, generator=g).double(), torch.rand(2000, generator=g).double()
        keep = MC.decided_to_basecolor_metallic(d, s, srgb, torch.ones(2000), torch.ones(2000))
        lin = MC._decode64(d) if srgb else d
        assert not bool((keep & ((lin - 0.04).abs() < 0.019) & (lin - 0.04 > 1e-5)).any()) and 0.5 < float(keep.double().mean()) < 1.0
