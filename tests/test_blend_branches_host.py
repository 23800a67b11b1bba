"""The branch fixture's BLEND mode (oracle/branch_cases.py: build_blend) held to its promises, on the CPU, with the oracles only: this is
where the inputs of tests/test_gpu_blend_branches.py get fixed.  For every blend variant -- every case of the render fixture with a signed
blended normal map, every case but `half_clamp` with a flat one (decoded again), and one variant with `degenerate` texels -- at every shape /
light set-up of branch_cases.BLEND_ENTRY_CONFIGS:

  * the branch the case names, the complementary branch and every promised sub-branch hold at least 10 % of the pixels, counted on decided
    pixels; at most 5 % of the pixels are undecided, the `degenerate` texels included;
  * mask 0 and mask 1 each sit on at least 10 % of the decided texels;
  * the whole-map "already signed?" flag is what the variant says;
  * the oracle's float64 gradients of both materials' maps and of the mask are finite everywhere, exactly 0 on back-lit pixels, exactly 0
    for material 2 where the mask is 1 and for material 1 where it is 0;
  * `decisions` on the blended maps rebuilds the oracle's rendering of the blend to 1e-14.

These caps are conditions on the inputs: a case that misses one gets other inputs, never another cap.
Run with -s to see each case's populations."""
import pytest
import torch

import blend_oracle as BO
import branch_cases as BC

VARIANTS = BC.all_blend_variants()
IDS = [BC.variant_id(n, kw) for n, kw in VARIANTS]


def _entries(kw):
    """The `degenerate` class is two 2 x 4 blocks and at most 2 % of the texels: it exists on the untiled 24 x 40 and 23 x 37 maps only."""
    return [e for e, cfg in BC.BLEND_ENTRY_CONFIGS.items() if not (kw.get("degenerate") and cfg[4] != 1)]


def _check_caps(case, tag):
    decided = BC.decided(case)
    kept = BC.unfold(decided, case.tile)
    for branch, mask in BC.branches(case).items():
        share = float((mask & kept).double().mean())
        assert share >= 0.10, (tag, branch, share)
    assert float((~decided).double().mean()) <= 0.05, tag
    for end in (0.0, 1.0):
        share = float((case.mask[0] == end)[decided].double().mean())
        assert share >= 0.10, (tag, "mask", end, share)


def _check_oracle_gradients(case, tag):
    ref, ref32 = BC.reference(case), BC.gradients(case, torch.float32)
    dark = BC.backlit(case)
    for name in case.map_names():
        assert bool(torch.isfinite(ref[name]).all()) and bool(torch.isfinite(ref32[name]).all()), (tag, name)
        assert bool((ref[name][:, dark] == 0).all()), (tag, name, "back-lit")
        if name[0] in "12":          # the material whose weight is 0
            unused = case.mask[0] == (0.0 if name[0] == "1" else 1.0)
            assert bool((ref[name][:, unused] == 0).all()), (tag, name, "weight 0")
    assert len(case.map_names()) == 9          # four maps of each material (metallic or specular) and the mask


@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_every_blend_populates_its_branch_and_stays_decided(name, kw):
    for entry in _entries(kw):
        case = BC.build_blend_for(entry, name, kw)
        tag = (BC.variant_id(name, kw), entry)
        print("%-24s flat %-5s mask 0 / 1 on %.1f / %.1f %% | %s" % (entry, case.flat, 100 * float((case.mask == 0).double().mean()),
                                                                     100 * float((case.mask == 1).double().mean()), BC.report(case)))
        _check_caps(case, tag)
        assert BC.blend_is_flat(case) == case.flat == bool(kw.get("flat", False)), tag
        _check_oracle_gradients(case, tag)
        if name == "backlit":
            assert float((BC.backlit(case) & BC.decided(case)).double().mean()) >= 0.10, tag
        share = float(case.degenerate.double().mean())
        assert (0 < share <= 0.02) if kw.get("degenerate") else share == 0, tag


def test_degenerate_texels_are_what_they_say():
    """Opposed unit normals under mask 0.5 (a blend of length exactly 0) and a stored normal of (0, 0, 0) in material 2, in 2 x 4 blocks;
    every one of them is kept out of `decided`, and the oracle's float32 gradients are finite there (so a kernel's must be)."""
    for entry in ("blend-pairs", "blend-one-pixel"):
        case = BC.build_blend_for(entry, "backview", dict(degenerate=True))
        (y0, x0), (y1, x1) = BC.DEGENERATE_BLOCKS
        a, b = (torch.nn.functional.normalize(m["normal"], dim=0) for m in (case.first, case.second))
        raw = case.mask * a + (1 - case.mask) * b
        assert bool((raw[:, y0:y0 + 2, x0:x0 + 4] == 0).all()) and bool((case.mask[:, y0:y0 + 2, x0:x0 + 4] == 0.5).all())
        assert bool((case.second["normal"][:, y1:y1 + 2, x1:x1 + 4] == 0).all())
        assert int(case.degenerate.sum()) == 16 and not bool((BC.decided(case) & case.degenerate).any())
        g32 = BC.gradients(case, torch.float32)
        assert all(bool(torch.isfinite(g32[n][:, case.degenerate]).all()) for n in case.map_names())


def test_batches_share_one_second_material_and_keep_the_caps():
    for entry, name, kw in BC.BLEND_BATCH_CASES:
        cases = BC.build_blend_batch(entry, name, kw)
        assert cases[1].second is cases[0].second and cases[1].mask is cases[0].mask
        assert not torch.equal(cases[0].first["albedo"], cases[1].first["albedo"])
        for b, case in enumerate(cases):
            tag = (entry, name, "material", b)
            _check_caps(case, tag)
            assert BC.blend_is_flat(case) == bool(kw.get("flat", False)), tag
            _check_oracle_gradients(case, tag)


def test_the_decisions_are_read_from_the_oracles_blend():
    """The case's own maps ARE blend_oracle.blend_materials of the two materials in float64, and `decisions`' pieces, clamped, summed and
    encoded as the oracle does, are the oracle's rendering of that blend (the one the gradients are taken through)."""
    for name, kw in VARIANTS:
        for entry in ("blend-one-pixel", "blend-multi-directional", "blend-tiled-point"):
            if entry not in _entries(kw):
                continue
            case = BC.build_blend_for(entry, name, kw)
            bl = BO.blend_materials(case.first, case.second, case.mask)
            for n, t in zip(BC.MAP_NAMES, case.maps()):
                assert (t is None and bl.get(n) is None) or torch.equal(t, bl[n]), (name, entry, n)
            t = BC._terms(case)
            colour = sum(u.clamp(0, 1) for u in t["u"]).clamp(0, 1)
            if case.return_srgb:
                colour = BC.O.linear_to_srgb(colour)
            assert (colour - BC.reference(case)["out"]).abs().max().item() <= 1e-14, (name, entry)


def test_blend_cases_are_deterministic_fp32_exact_and_differ_by_seed():
    for kw in (dict(), dict(flat=True)):
        a, b, c = (BC.build_blend("saturated", 24, 40, n_lights=3, seed=s, **kw) for s in (0, 0, 2))
        for key in ("first", "second"):
            for n, x in getattr(a, key).items():
                assert torch.equal(x, getattr(b, key)[n]) and not torch.equal(x, getattr(c, key)[n]), (key, n)
                assert x.dtype == torch.float64 and torch.equal(x, x.float().double()), (key, n)
        assert torch.equal(a.mask, b.mask) and torch.equal(a.mask, a.mask.float().double()) and torch.equal(a.weight, b.weight)
        assert set(a.mask.unique().tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}
        # the two materials differ: normals by 5 to 12 degrees where the mask is inside (0, 1), stored at two lengths
        n1, n2 = (torch.nn.functional.normalize(m["normal"], dim=0) for m in (a.first, a.second))
        angle = torch.rad2deg(torch.acos((n1 * n2).sum(0).clamp(-1, 1)))
        assert 4.9 <= float(angle.min()) and float(angle.max()) <= 12.1
        assert abs(float(a.first["normal"].norm(dim=0).mean()) - 0.75) < 1e-6 and abs(float(a.second["normal"].norm(dim=0).mean()) - 1.25) < 1e-6
