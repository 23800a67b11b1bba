"""The branch fixture in STACK mode (oracle/branch_cases.py, stack=True) held to its promises, on the CPU, with the float64 oracle only:
the counterpart of test_branch_cases_host.py for the light stack (csrc/ct_stack.hip), whose step runs the one-light chain rule inside
a light loop -- every light with its own clamp, encode, target and upstream gradient.  For every variant (the summed-lights ones read
as a stack, plus `split_lights`) at every entry of branch_cases.STACK_ENTRY_CONFIGS:

  * every branch and sub-branch holds at least 10 % of the pixels, counted on decided pixels, and at most 5 % are undecided;
  * the oracle's gradients are finite, and exactly 0 where every light is behind;
  * the stack rebuilt from the pieces `decisions` reads (each u[l] clamped, then encoded) is the oracle's stack to 1e-14;
  * stack=True builds the inputs the summed-lights case has: maps, lights and view are torch.equal, and so are the intensities except
    for `saturated` and `closed_ends`, which are lit differently in stack mode (branch_cases.STACK_INTENSITIES says why);
  * the MSE targets of the GPU test (branch_cases.stack_target: the stack of the seed ^ 1 material; for `dark` light 1's target is
    light 0's image, because the case's own lights 1 and 2 are behind everywhere and render 0 at every seed) have bite: out - target
    is above 1e-3 on at least 5 % of the elements and below -1e-3 on at least 5 %, and for `split_lights`, `backlit` and `dark` the
    target exceeds 1e-3 in some channel on at least 10 % of the (pixel, light) pairs whose light is decided behind -- the term that
    must be masked.  Held at seed 0 and, for the two-material batch of the GPU test, at seed 1.

Run with -s to see each case's populations."""
import pytest
import torch

import branch_cases as BC
from test_branch_cases_host import _check_caps

VARIANTS = BC.all_stack_variants()
IDS = [BC.variant_id(n, kw) for n, kw in VARIANTS]
MASKED_TERM_CASES = ("split_lights", "backlit", "dark")
BATCH_ENTRIES = ("stack-pairs", "stack-fp16")          # where the GPU test runs `split_lights` as a batch of seeds 0 and 1


def _check_bite(entry, name, kw, seed):
    case = BC.build_for(entry, name, kw, seed=seed)
    target = BC.stack_target(entry, name, kw, seed=seed).double()
    diff = BC.render(case) - target
    up, down = float((diff > 1e-3).double().mean()), float((diff < -1e-3).double().mean())
    assert up >= 0.05 and down >= 0.05, (entry, name, seed, up, down)
    if name in MASKED_TERM_CASES:
        behind = BC.behind(case)                                   # [L,H,W]
        assert bool(behind.any()), (entry, name, seed)
        share = float((target > 1e-3).any(dim=1)[behind].double().mean())
        print("%-18s seed %d: out - target > 1e-3 on %.1f%%, < -1e-3 on %.1f%%; target > 1e-3 on %.1f%% of the (pixel, light) pairs behind"
              % (entry, seed, 100 * up, 100 * down, 100 * share))
        assert share >= 0.10, (entry, name, seed, share)


@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_every_stack_case_populates_its_branches_and_stays_decided(name, kw):
    for entry in BC.STACK_ENTRY_CONFIGS:
        case = BC.build_for(entry, name, kw)
        assert case.stack and case.n_lights == 3 and case.tile == 1
        print("%-18s %s" % (entry, BC.report(case)))
        _check_caps(case, entry)
        ref = BC.reference(case)
        assert ref["out"].shape == (3, 3) + case.out_shape
        dark = BC.backlit(case)
        for m in case.map_names():
            assert bool(torch.isfinite(ref[m]).all()), (entry, m)
            assert bool((ref[m][:, dark] == 0).all()), (entry, m)
        if name == "backlit":
            assert float((dark & BC.decided(case)).double().mean()) >= 0.10, entry
        _check_bite(entry, name, kw, 0)
        if name == "split_lights" and entry in BATCH_ENTRIES:
            _check_caps(BC.build_for(entry, name, kw, seed=1), entry + " seed 1")
            _check_bite(entry, name, kw, 1)


def test_the_stack_rebuilt_from_the_decisions_pieces_is_the_oracle():
    for name, kw in VARIANTS:
        for entry in ("stack-pairs", "stack-one-pixel"):
            case = BC.build_for(entry, name, kw)
            stack = torch.stack([u.clamp(0, 1) for u in BC._terms(case)["u"]])
            if case.return_srgb:
                stack = BC.O.linear_to_srgb(stack)
            assert (stack - BC.render(case)).abs().max().item() <= 1e-14, (name, entry)
            # a stack case has one knee per light and no summed colour among its decisions
            listed = [d[0] for d in BC.decisions(case)]
            assert "sum vs 1" not in listed and ("colour[2] vs knee" in listed) == case.return_srgb


def test_stack_mode_leaves_the_inputs_of_the_existing_cases_untouched():
    for name, kw in BC.all_variants():
        for entry, (h, w, light_type, n_lights, _) in BC.STACK_ENTRY_CONFIGS.items():
            for seed in (0, 1):
                stack = BC.build_for(entry, name, kw, seed=seed)
                plain = BC.build(name, h, w, light_type=light_type, n_lights=n_lights, seed=seed, **kw)
                assert stack.stack and not plain.stack
                for x, y in zip(stack.maps(), plain.maps()):
                    assert (x is None and y is None) or torch.equal(x, y), (name, entry)
                assert torch.equal(stack.lights, plain.lights) and torch.equal(stack.view, plain.view), (name, entry)
                assert torch.equal(stack.intensities, plain.intensities) == (name not in BC.STACK_INTENSITIES), (name, entry)
    assert sorted(BC.STACK_INTENSITIES) == ["closed_ends", "saturated"]


def test_a_light_behind_renders_exactly_zero_and_saturated_lights_straddle_the_clamp():
    """What the GPU test asserts exactly: the image of a light decided behind is 0 in the oracle (linear_to_srgb(0) = 0 when encoded);
    and in `saturated` the named pixels have light 0 clamped where light 1 or 2 is not."""
    for kw in BC.VARIANTS["split_lights"]:
        case = BC.build_for("stack-one-pixel", "split_lights", kw)
        out, behind = BC.render(case), BC.behind(case)
        assert float(BC.O.linear_to_srgb(torch.zeros(1, dtype=torch.float64))) == 0.0
        assert bool((out.permute(1, 0, 2, 3)[:, behind] == 0).all())
    case = BC.build_for("stack-pairs", "saturated", {})
    u = BC._terms(case)["u"]
    named = BC.branches(case)["named"]
    assert bool(((u[0] > 1).any(0) & ((u[1] < 1).all(0) | (u[2] < 1).all(0)))[named].all())
