"""The branch fixture (oracle/branch_cases.py) held to its promises, on the CPU, with the float64 oracle only: this is where the
inputs of the GPU gradient-branch tests get fixed.  For every case, at every shape / light set-up of branch_cases.ENTRY_CONFIGS:

  * the branch the case names holds at least 10 % of the pixels, and so does the complementary branch (and every sub-branch
    the case promises: each decode region of `albedo_range`, each closed end of `closed_ends`, 'one light saturates alone'
    and 'saturates only in the sum' of the three-light `saturated`);
  * at most 5 % of the pixels are undecided -- within 1e-3 of a threshold, or ill-conditioned (the oracle's own float32
    gradient further than half the band from its float64 gradient);
  * the oracle's gradient is exactly 0 on back-lit pixels and finite everywhere.

`closed_ends`: all four ends survive.  On every texel that stores albedo 0.0, albedo 1.0, metallic 0 or metallic 1, at every set-up,
the oracle's float32 and float64 gradients agree within half the band (torch's clamp passes the gradient at both ends in either
precision, and ((1.0 + 0.055) / 1.055) ** 2.4 does not exceed 1 in either), so no end is left out; test_all_closed_ends_survive
asserts it.  Run with -s to see each case's populations."""
import pytest
import torch

import branch_cases as BC

VARIANTS = BC.all_variants()
IDS = [BC.variant_id(n, kw) for n, kw in VARIANTS]


def _check_caps(case, entry):
    """Populations are counted on DECIDED pixels only: the undecided 5 % may not be what fills a (sub-)branch."""
    kept = BC.unfold(BC.decided(case), case.tile)
    for branch, mask in BC.branches(case).items():
        share = float((mask & kept).double().mean())
        assert share >= 0.10, (entry, branch, share)
    assert float((~BC.decided(case)).double().mean()) <= 0.05, entry


@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_every_case_populates_its_branch_and_stays_decided(name, kw):
    for entry in BC.ENTRY_CONFIGS:
        case = BC.build_for(entry, name, kw)
        print("%-24s %s" % (entry, BC.report(case)))
        _check_caps(case, entry)
        ref = BC.reference(case)
        dark = BC.backlit(case)
        for m in case.map_names():
            assert bool(torch.isfinite(ref[m]).all()), (entry, m)
            assert bool((ref[m][:, dark] == 0).all()), (entry, m)
        if name == "backlit":
            assert float((dark & BC.decided(case)).double().mean()) >= 0.10, entry
    # the one-tile fp16 launch is the 128-wide case cut to 120 columns: the cut keeps the caps, and its decisions are the slice's
    wide = BC.build_for("fp16-streamed", name, kw)
    cut = BC.crop(wide, 120)
    _check_caps(cut, "fp16 one-tile (120 of 128 columns)")
    assert torch.equal(BC.threshold_decided(cut), BC.threshold_decided(wide)[:, :120])


def test_the_pieces_the_decisions_are_read_from_are_the_oracle():
    """`decisions` rebuilds the per-light contribution from torch_oracle's own functions; clamped, summed and encoded as the
    oracle does, it must BE the oracle's rendering."""
    for name, kw in VARIANTS:
        for entry in ("fp32-one-pixel", "multi-directional", "tiled-point"):
            case = BC.build_for(entry, name, kw)
            t = BC._terms(case)
            colour = sum(u.clamp(0, 1) for u in t["u"]).clamp(0, 1)
            if case.return_srgb:
                colour = BC.O.linear_to_srgb(colour)
            assert (colour - BC.render(case)).abs().max().item() <= 1e-14, (name, entry)


def test_cases_are_deterministic_fp16_exact_and_differ_by_seed():
    a, b, c = (BC.build("saturated", 24, 40, n_lights=3, seed=s) for s in (0, 0, 1))
    for x, y, z in zip(a.maps(), b.maps(), c.maps()):
        if x is not None:
            assert torch.equal(x, y) and not torch.equal(x, z)
            assert torch.equal(x, x.half().double())
    assert torch.equal(a.weight, b.weight)


def test_filling_undecided_pixels_leaves_none():
    """The view / light / intensity gradients are sums over all pixels: their tests run on the case with every undecided texel
    replaced by a decided neighbour's values."""
    for name, kw in VARIANTS:
        for entry in ("fp32-vector-lanes-point", "multi-directional"):
            filled, left = BC.fill_undecided(BC.build_for(entry, name, kw))
            assert left == 0.0, (name, entry, left)
            _check_caps(filled, entry)


def test_all_closed_ends_survive():
    """Every texel with an exactly representable end (albedo 0.0 / 1.0, metallic 0 / 1) is well conditioned, and at least 90 % of each
    end's texels are decided (the rest fail another threshold, e.g. a contribution next to 1)."""
    for entry in BC.ENTRY_CONFIGS:
        case = BC.build_for(entry, "closed_ends", {})
        a, m = case.albedo, case.metallic[0]
        for end, mask in (("albedo 0", (a == 0).any(0)), ("albedo 1", (a == 1).any(0)), ("metallic 0", m == 0), ("metallic 1", m == 1)):
            assert bool(BC.well_conditioned(case)[mask].all()), (entry, end)
            assert float(BC.decided(case)[mask].double().mean()) >= 0.90, (entry, end)
