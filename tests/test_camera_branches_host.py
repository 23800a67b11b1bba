"""The branch fixture in CAMERA mode (oracle/branch_cases.py, camera="fixed" | "per_shot") held to its promises, on the CPU, with the float64
oracle only: the counterpart of test_branch_cases_host.py and test_light_stack_branches_host.py for the perspective camera (csrc/ct_camera.hip,
ct_camera_stack.hip, ct_view_stack.hip), whose kernels run the chain rule over a per-pixel view -- N.V and N.H change sign from pixel to pixel
inside one lane group, and with one camera per shot a shot seen from behind and a shot seen from the front add into one pixel adjoint.  For
every variant at every entry of branch_cases.CAMERA_ENTRY_CONFIGS that runs it:

  * the named branch, the complement and every listed sub-branch hold at least 10 % of the pixels, counted on decided pixels, at most 5 % are
    undecided, and `backlit` keeps at least 10 % back-lit and decided;
  * `split_views`: every shot is seen from behind on at least 10 % of the pixels, and every count of front-facing shots from 1 to L holds
    at least 10 % (its sub-branches from_behind_l, one_front, two_front and the complement, all L in front);
  * the oracle's gradients are finite, and exactly 0 where every light is behind;
  * the MSE targets of the GPU test (branch_cases.camera_target: another seed) have bite: out - target is above 1e-3 on at least 5 % of the
    elements and below -1e-3 on at least 5 %; in a stack the target exceeds 1e-3 on at least 10 % of the (pixel, light) pairs decided behind;
  * the render rebuilt from the pieces `decisions` reads is the oracle's to 1e-14;
  * with one view forced on every pixel a camera case IS the orthographic case, bit for bit;
  * `fill_undecided` leaves none undecided, and on the filled cases the oracle's own float32 gradients of camera, lights and intensities lie
    within HALF the band the GPU test uses (test_gpu_camera._param_band: 2e-5 S + 1e-9), so that band is no guess;
  * camera mode leaves the inputs of the build without a camera untouched (all but the normals, which skip angles against the per-pixel dots,
    and `dark`'s albedo, which is solved under the view it is rendered with).

Run with -s to see each case's populations."""
import pytest
import torch

import branch_cases as BC
from test_branch_cases_host import _check_caps

VARIANTS = BC.all_view_stack_variants()
IDS = [BC.variant_id(n, kw) for n, kw in VARIANTS]
MASKED_TERM_CASES = ("split_lights", "backlit", "dark")
# where the GPU test takes parameter gradients (fill_undecided cases), and where it runs a batch of seeds 0 and 1
PARAM_ENTRIES = ("camera-vector-lanes-point", "camera-multi-directional", "camera-stack-pairs-point", "camera-stack-pairs",
                 "view-stack-pairs-point", "view-stack-one-pixel")
BATCH_CASES = (("camera-stack-pairs-point", "split_lights"), ("view-stack-pairs-point", "split_views"), ("view-stack-fp16", "split_views"))


def param_band(want):
    """test_gpu_camera._param_band, the rule the camera kernels were accepted under (that module needs no device to import, but it pulls in
    the GPU helpers; the rule is two numbers)."""
    return 2e-5 * max(float(want[k].abs().max()) for k in ("view", "lights", "intensities")) + 1e-9


def runs(entry, name):
    return name in {n for n, _ in BC.camera_variants(entry)}


def _check_bite(entry, name, kw, seed):
    case = BC.build_for(entry, name, kw, seed=seed)
    target = BC.camera_target(entry, name, kw, seed=seed).double()
    diff = BC.render(case) - target
    up, down = float((diff > 1e-3).double().mean()), float((diff < -1e-3).double().mean())
    assert up >= 0.05 and down >= 0.05, (entry, name, seed, up, down)
    if case.stack and name in MASKED_TERM_CASES:
        behind = BC.behind(case)                                   # [L,H,W]
        share = float((target > 1e-3).any(dim=1)[behind].double().mean())
        assert bool(behind.any()) and share >= 0.10, (entry, name, seed, share)


@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_every_camera_case_populates_its_branches_and_stays_decided(name, kw):
    for entry, (h, w, light_type, n_lights, _, mode) in BC.CAMERA_ENTRY_CONFIGS.items():
        if not runs(entry, name):
            continue
        case = BC.build_for(entry, name, kw)
        assert case.camera.shape == ((n_lights, 3) if mode == "view_stack" else (3,)) and torch.equal(case.camera, case.camera.float().double())
        assert case.light_size == 1.0 and case.stack == (mode != "sum") and case.tile == 1 and case.product_kwargs()["view_type"] == "point"
        print("%-26s %s" % (entry, BC.report(case)))
        _check_caps(case, entry)
        ref = BC.reference(case)
        assert ref["out"].shape == ((3,) if mode == "sum" else (n_lights, 3)) + (h, w)
        dark = BC.backlit(case)
        for m in case.map_names():
            assert bool(torch.isfinite(ref[m]).all()), (entry, m)
            assert bool((ref[m][:, dark] == 0).all()), (entry, m)
        if name == "backlit":
            assert float((dark & BC.decided(case)).double().mean()) >= 0.10, entry
        if name == "split_views":
            b = BC.branches(case)
            assert sorted(b) == ["complement", "from_behind_0", "from_behind_1", "from_behind_2", "named", "one_front", "two_front"]
            listed = [d[0] for d in BC.decisions(case)]
            assert all("n.v[%d]" % l in listed for l in range(3)) and "n.v" not in listed
        _check_bite(entry, name, kw, 0)
        if (entry, name) in BATCH_CASES:
            _check_caps(BC.build_for(entry, name, kw, seed=1), entry + " seed 1")
            _check_bite(entry, name, kw, 1)


def test_the_pieces_the_decisions_are_read_from_are_the_camera_oracle():
    """`decisions` rebuilds every light's contribution from torch_oracle's pieces over the per-pixel view map (of its shot); clamped, summed
    (or stacked) and encoded as the oracle does, it must BE tools/camera_oracle.py's rendering."""
    for entry in ("camera-one-pixel", "camera-multi-directional", "camera-stack-pairs-point", "view-stack-one-pixel", "view-stack-pairs"):
        for name, kw in BC.camera_variants(entry):
            case = BC.build_for(entry, name, kw)
            u = BC._terms(case)["u"]
            colour = torch.stack([x.clamp(0, 1) for x in u]) if case.stack else sum(x.clamp(0, 1) for x in u).clamp(0, 1)
            if case.return_srgb:
                colour = BC.O.linear_to_srgb(colour)
            assert (colour - BC.render(case)).abs().max().item() <= 1e-14, (name, entry)
            listed = [d[0] for d in BC.decisions(case)]
            assert ("n.v[1]" in listed) == case.per_shot and ("n.v" in listed) != case.per_shot


def test_one_view_forced_on_every_pixel_is_the_orthographic_case():
    """The camera's rendering with every pixel's view forced to normalize(case.view) against the SAME maps, lights and intensities read without a
    camera (torch_oracle): bit for bit in float64, for one light, three summed lights and the stack."""
    for entry in ("camera-vector-lanes", "camera-one-pixel", "camera-multi-point", "camera-stack-pairs-point", "view-stack-pairs"):
        for name, kw in BC.camera_variants(entry):
            case = BC.build_for(entry, name, kw)
            H, W = case.out_shape
            forced = torch.nn.functional.normalize(case.view, dim=0).view(3, 1, 1).expand(3, H, W)
            plain = case.replace(camera=None)
            assert plain.camera is None
            assert torch.equal(BC.render(case, view_map=forced), BC.render(plain)), (name, entry)
    # and the camera does matter: without the forced view the rendering differs by more than 1e-3 somewhere
    case = BC.build_for("camera-vector-lanes", "backview", {})
    assert float((BC.render(case) - BC.render(case.replace(camera=None))).abs().max()) > 1e-3


@pytest.mark.parametrize("name,kw", VARIANTS, ids=IDS)
def test_filling_undecided_pixels_leaves_none_and_the_parameter_band_has_room(name, kw):
    """The gradients of camera, lights and intensities are sums over all pixels: their GPU tests run on the case with every undecided texel
    replaced by a decided neighbour's values.  There the oracle's own float32 parameter gradients must lie within half the GPU test's band --
    for sum(out * W) (cook_torrance) and, in a stack, for the N / 2-scaled MSE against the other seed's target (the fit steps)."""
    for entry in PARAM_ENTRIES:
        if not runs(entry, name):
            continue
        filled, left = BC.fill_undecided(BC.build_for(entry, name, kw))
        assert left == 0.0, (name, entry, left)
        _check_caps(filled, entry)
        target = BC.camera_target(entry, name, kw).double() if filled.stack else None
        scale = 1.0 if target is None else target.numel() / 2.0
        g64 = BC.gradients(filled, params=True, loss_target=target)
        g32 = BC.gradients(filled, torch.float32, params=True, loss_target=target)
        band = param_band({k: g64[k] * scale for k in ("view", "lights", "intensities")})
        assert g64["view"].shape == filled.camera.shape
        for k in ("view", "lights", "intensities"):
            err = float((g32[k].double() - g64[k]).abs().max()) * scale
            print("%-26s %-12s %-11s float32 oracle error / band %.4f" % (entry, name, k, err / band))
            assert err <= 0.5 * band, (entry, name, k, err, band)


def test_camera_mode_leaves_the_inputs_of_the_existing_cases_untouched():
    for entry, (h, w, light_type, n_lights, _, mode) in BC.CAMERA_ENTRY_CONFIGS.items():
        for name, kw in BC.camera_variants(entry):
            if name == "split_views":
                continue
            for seed in (0, 1):
                cam = BC.build_for(entry, name, kw, seed=seed)
                plain = BC.build(name, h, w, light_type=light_type, n_lights=n_lights, seed=seed, stack=mode != "sum", **kw)
                assert cam.camera is not None and plain.camera is None and "view_type" not in plain.product_kwargs()
                for m, x, y in zip(BC.MAP_NAMES, cam.maps(), plain.maps()):
                    if m == "normal" or (m == "albedo" and name == "dark"):
                        assert x.shape == y.shape and torch.equal(x, x.half().double())
                        continue
                    assert (x is None and y is None) or torch.equal(x, y), (name, entry, m)
                assert torch.equal(cam.lights, plain.lights) and torch.equal(cam.view, plain.view), (name, entry)
                assert torch.equal(cam.intensities, plain.intensities) and torch.equal(cam.weight, plain.weight), (name, entry)
                assert plain.light_size == (1.0 if light_type == "point" else None)
    # the one case whose camera and tilt range are its own (branch_cases.CAMERA_PLACES says why)
    assert sorted(BC.CAMERA_PLACES) == sorted(BC.CAMERA_TILTS) == ["half_clamp"]


def test_camera_cases_are_deterministic_and_differ_by_seed():
    a, b, c = (BC.build_for("view-stack-one-pixel", "split_views", dict(return_srgb=True), seed=s) for s in (0, 0, 1))
    for x, y, z in zip(a.maps(), b.maps(), c.maps()):
        if x is not None:
            assert torch.equal(x, y) and not torch.equal(x, z) and torch.equal(x, x.half().double())
    assert torch.equal(a.camera, b.camera) and torch.equal(a.camera, c.camera) and torch.equal(a.weight, b.weight)
    front = [(v[0] > 0) for v in BC._terms(a)["ndv_l"]]
    assert not torch.equal(front[0], front[1]) and not torch.equal(front[1], front[2])
