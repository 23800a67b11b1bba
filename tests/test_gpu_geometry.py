"""The geometric material transforms on the GPU (csrc/geometry.hip): crop, flips, roll, tile and chains of them as one index map.

Forward values are COPIES (a negated plane has its sign flipped), so every forward comparison is torch.equal: against the real reference's
outputs (tests/golden/geometry.npz, tools/gen_geometry_golden.py) through the MaterialBase methods and through pypbr_amd.transforms, and
against ATen indexing on the device at the shapes where quad alignment, the wrap inside a quad, the reversed quad and the 256-pixel strip
edge can go wrong.  Gradients of chains without a tile are permutations with zeros: bit-equal to float64 autograd through the ATen chain;
with a tile at most 9 fp32 terms are summed: within the suite's 2e-5 (1 + |g|) band."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from test_gpu_write_guards import Guards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_geometry_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "geometry.npz"))
LIGHT = dict(view=torch.tensor([0.0, 0.0, 1.0]), light=torch.tensor([0.1, 0.1, 1.0]), intensity=torch.tensor([1.0, 1.0, 1.0]))


def _gold(prefix, dtype=torch.float32):
    return {k: torch.from_numpy(GOLD["%s__%s" % (prefix, k)]).to(dtype) for k in G.MAPS}


def _material(maps, requires_grad=()):
    from pypbr_amd.materials import BasecolorMetallicMaterial
    dev = {k: v.cuda() for k, v in maps.items()}
    for k in requires_grad:
        dev[k].requires_grad_()
    return BasecolorMetallicMaterial(**dev)


def aten_stages(t, stages, normal=False):
    """The reference's own ATen chain (base.py:506-537, :605-655) on a [..., C, H, W] tensor, on whatever device / dtype it has."""
    for st in stages:
        if st[0] == "flip_h":
            t = t.flip(-1)
            if normal:
                t = torch.cat([-t[..., 0:1, :, :], t[..., 1:, :, :]], dim=-3)
        elif st[0] == "flip_v":
            t = t.flip(-2)
            if normal:
                t = torch.cat([t[..., 0:1, :, :], -t[..., 1:2, :, :], t[..., 2:, :, :]], dim=-3)
        elif st[0] == "crop":
            top, left, h, w = st[1:]
            t = t[..., top:top + h, left:left + w]
        elif st[0] == "roll":
            t = torch.roll(t, (st[1], st[2]), dims=(-2, -1))
        elif st[0] == "tile":
            t = t.repeat(*((1,) * (t.dim() - 2) + (st[1], st[2])))
    return t


def run_stages(t, stages, normal=False):
    """The stages folded on the host and run through functional.remap_planes, map after map."""
    from pypbr_amd import functional as F
    for pm in F.fold_stages(t.shape[-2], t.shape[-1], stages):
        t = F.remap_planes(t, pm.ymap, pm.xmap, negate=[p for p, on in zip((0, 1), pm.neg) if on] if normal else (), out_size=pm.size)
    return t


def as_transforms(stages):
    from pypbr_amd import transforms as T
    out = []
    for st in stages:
        out.append({"flip_h": lambda: T.FlipHorizontal(), "flip_v": lambda: T.FlipVertical(), "crop": lambda: T.Crop(*st[1:]),
                    "roll": lambda: T.Roll((st[1], st[2])), "tile": lambda: T.Tile(st[1])}[st[0]]())
    return out


# ---- golden cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("via", ["methods", "transforms", "functional"])
def test_every_golden_case(via, dtype):
    from pypbr_amd import transforms as T
    for case, (m, stages) in G.CASES.items():
        ins, want = _gold("in__" + m, dtype), _gold("out__" + case, dtype)
        mat = _material(ins)
        if stages[0][0] == "random":
            random.seed(stages[0][1])
            run = [T.RandomCrop(*G.RANDOM_CROP), T.RandomHorizontalFlip(), T.RandomVerticalFlip()]
            if via == "functional":                   # stage by stage, as upstream's Compose
                out = mat
                for tr in run:
                    out = tr(out)
            else:
                out = T.Compose(run, fuse=(via == "transforms"))(mat)
        elif via == "methods":
            out = G.apply_stages(mat, stages)
            assert out is mat
        elif via == "transforms":
            out = T.Compose(as_transforms(stages))(mat)
        else:
            out = mat
            for tr in as_transforms(stages):
                out = tr(out)
        for k in G.MAPS:
            got = out._maps[k]
            assert got.dtype == dtype and got.is_cuda, (case, k)
            assert got.shape == want[k].shape and torch.equal(got.cpu(), want[k]), (via, case, k)
        if via != "methods":                           # the transforms leave their argument as it was
            for k in G.MAPS:
                assert torch.equal(mat._maps[k].cpu(), ins[k]), (via, case, k)


def test_cpu_resident_material_goes_through_the_device():
    ins, want = _gold("in__37x53"), _gold("out__37x53__chain_b")
    from pypbr_amd.materials import BasecolorMetallicMaterial
    mat = BasecolorMetallicMaterial(**{k: v.clone() for k, v in ins.items()})
    G.apply_stages(mat, G.CASES["37x53__chain_b"][1])
    for k in G.MAPS:
        assert mat._maps[k].device.type == "cpu" and torch.equal(mat._maps[k], want[k]), k


# ---- forward against ATen -------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260, 1023)
HEIGHTS = (1, 2, 7)


def _cases_for(H, W):
    offs = sorted({0, 1 % W, 2 % W, 3 % W, W - 1})
    shifts = (0, 1, 2, 3, W - 1, W + 5)
    cases = [[("flip_h",)], [("flip_v",)], [("flip_h",), ("flip_v",)], [("tile", 2, 2)]]
    cases += [[("roll", s % 3, s)] for s in shifts] + [[("roll", -s, -s)] for s in shifts[1:]]
    cases += [[("crop", min(o, H - 1), o, H - min(o, H - 1), W - o)] for o in offs]
    cases += [[("crop", 0, o, H, 1)] for o in offs] + [[("crop", 0, 0, H, max(1, W - o))] for o in offs]
    cases += [[("roll", 1, s), ("tile", 3, 3)] for s in shifts]
    cases += [[("flip_h",), ("roll", 0, s)] for s in shifts]
    cases += [[("roll", 2, s), ("flip_h",), ("crop", 0, o, H, W - o), ("flip_v",)] for s, o in zip(shifts, offs)]
    cases += [[("flip_h",), ("crop", 0, o, H, W - o), ("tile", 2, 3), ("roll", 1, W + 5)] for o in offs]      # the tile may not fold
    return cases


@pytest.mark.parametrize("W", WIDTHS)
def test_forward_equals_aten_indexing(W):
    g = torch.Generator().manual_seed(W)
    for H in HEIGHTS:
        t = (torch.rand(5, H, W, generator=g) - 0.5).cuda()
        normal = (torch.rand(3, H, W, generator=g) - 0.5).cuda()
        for stages in _cases_for(H, W):
            want = aten_stages(t, stages)
            got = run_stages(t, stages)
            assert got.shape == want.shape and torch.equal(got, want), (H, W, stages)
            assert torch.equal(run_stages(normal, stages, True), aten_stages(normal, stages, True)), ("normal", H, W, stages)
        h16 = t.half()
        for stages in _cases_for(H, W)[::4]:
            assert torch.equal(run_stages(h16, stages), aten_stages(h16, stages)), ("fp16", H, W, stages)


@pytest.mark.parametrize("W", (5, 64, 257))
def test_every_offset_and_step_of_one_map(W):
    from pypbr_amd import functional as F
    H = 3
    t = torch.arange(2 * H * W, dtype=torch.float32).reshape(2, H, W).cuda() + 1.0
    for ox in sorted({0, 1 % W, 2 % W, 3 % W, W // 2, W - 1}):
        for sx in (1, -1):
            for oy, sy in ((0, 1), (H - 1, -1), (1, 1)):
                for ho, wo in ((H, W), (2 * H + 1, W + 3), (1, max(1, W - 2))):
                    rows = torch.tensor([(oy + sy * i) % H for i in range(ho)], device="cuda")
                    cols = torch.tensor([(ox + sx * j) % W for j in range(wo)], device="cuda")
                    want = t.index_select(1, rows).index_select(2, cols).clone()
                    want[1] = -want[1]
                    got = F.remap_planes(t, (oy, sy), (ox, sx), negate=(1,), out_size=(ho, wo))
                    assert torch.equal(got, want), (W, ox, sx, oy, sy, ho, wo)


def test_a_4096_square_block_of_nine_planes():
    g = torch.Generator(device="cuda").manual_seed(3)
    block = torch.rand(9, 4096, 4096, device="cuda", generator=g) - 0.5
    stages = [("roll", 1, 1), ("flip_h",), ("crop", 1023, 2047, 2048, 2048), ("flip_v",), ("roll", 2048, 0)]
    from pypbr_amd import functional as F
    maps = F.fold_stages(4096, 4096, stages)
    assert len(maps) == 1
    pm = maps[0]
    got = F.remap_planes(block, pm.ymap, pm.xmap, negate=[3 + p for p in (0, 1) if pm.neg[p]], out_size=pm.size)
    want = torch.cat([aten_stages(block[:3], stages), aten_stages(block[3:6], stages, True), aten_stages(block[6:], stages)])
    assert got.shape == (9, 2048, 2048) and torch.equal(got, want)
    del got, want
    whole = F.remap_planes(block, (1, 1), (4095, -1))            # a full-size reversed pass with an odd row offset
    assert torch.equal(whole, torch.roll(block, -1, dims=1).flip(-1))


# ---- batches --------------------------------------------------------------------------------------------------------------------------
def test_batch_images_are_independent_and_strided_blocks_work():
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(11)
    x = torch.rand(5, 4, 23, 70, generator=g).cuda()
    out = F.remap_planes(x, (3, -1), (9, 1), negate=(1, 3), out_size=(30, 81))
    for b in range(5):
        assert torch.equal(out[b], F.remap_planes(x[b], (3, -1), (9, 1), negate=(1, 3), out_size=(30, 81))), b
    assert not torch.equal(out[0], out[1])
    big = torch.rand(3, 9, 23, 70, generator=g).cuda()
    view = big[1:, 2:8:2]                                         # batch and plane strides that are not the dense ones
    assert not view.is_contiguous() and view.stride(-1) == 1 and view.stride(-2) == 70
    got = F.remap_planes(view, (0, 1), (69, -1), negate=(0,))
    want = view.flip(-1).clone()
    want[:, 0] = -want[:, 0]
    assert torch.equal(got, want)
    lead = torch.rand(2, 3, 2, 7, 9, generator=g).cuda()          # [..., P, H, W]
    assert torch.equal(F.remap_planes(lead, (6, -1), (0, 1)), lead.flip(-2))


def test_the_32_plane_limit():
    from pypbr_amd import _native as N, functional as F
    x = torch.rand(33, 6, 10).cuda()
    got = F.remap_planes(x[:32], (0, 1), (9, -1), negate=(0, 31))
    want = x[:32].flip(-1).clone()
    want[0], want[31] = -want[0], -want[31]
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        F.remap_planes(x, (0, 1), (9, -1))
    out = torch.empty_like(x)
    s = torch.cuda.current_stream().cuda_stream
    args = (x.data_ptr(), 0, 60, out.data_ptr(), 0, 60, 1)
    assert N.lib().pbr_remap_planes(*args, 33, 6, 10, 6, 10, 0, 1, 9, -1, 0, N.F32, s) == N.ERR_SHAPE
    assert N.lib().pbr_remap_planes(*args, 32, 6, 10, 6, 10, 0, 1, 10, -1, 0, N.F32, s) == N.ERR_SHAPE      # offset outside the row
    assert N.lib().pbr_remap_planes(*args, 32, 6, 10, 6, 10, 0, 2, 9, -1, 0, N.F32, s) == N.ERR_SHAPE       # a step that is not +-1
    assert N.lib().pbr_remap_planes(*args, 32, 6, 10, 6, 10, 0, 1, 9, -1, 0, 7, s) == N.ERR_DTYPE
    assert N.lib().pbr_remap_planes_backward(*args, 33, 6, 10, 6, 10, 0, 1, 9, -1, 0, s) == N.ERR_SHAPE
    assert N.lib().pbr_remap_planes(*args, 32, 6, 10, 6, 10, 0, 1, 9, -1, 0, N.F32, s) == N.OK


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(37, 53), (5, 1), (1, 9), (70, 260)]


def _window(H, W):
    return (H // 4, W // 3, max(1, H // 2), max(1, W // 2))


def _grad_pair(H, W, stages, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(3, H, W, generator=g) - 0.5
    x64 = x.double().requires_grad_()
    ref = aten_stages(x64, stages, True)
    weight = torch.randn(ref.shape, generator=g)
    (ref * weight.double()).sum().backward()
    xd = x.cuda().requires_grad_()
    out = run_stages(xd, stages, True)
    assert torch.equal(out.detach().cpu(), ref.detach().float())
    (out * weight.cuda()).sum().backward()
    return xd.grad.cpu(), x64.grad


@pytest.mark.parametrize("hw", SHAPES)
def test_gradients_of_chains_without_a_tile_are_exact(hw):
    H, W = hw
    win = _window(H, W)
    chains = [[("flip_h",)], [("flip_v",)], [("roll", 3, -5)], [("crop",) + win],
              [("roll", 1, W + 5), ("flip_h",), ("crop",) + win, ("flip_v",)],
              [("crop",) + win, ("roll", 2, 3), ("flip_h",)]]
    for i, stages in enumerate(chains):
        got, want = _grad_pair(H, W, stages, 100 + i)
        assert torch.equal(got, want.float()), (hw, stages)
    # a crop's gradient is exactly 0 outside its window (and the window holds the weights)
    got, _ = _grad_pair(H, W, [("crop",) + win], 7)
    outside = torch.ones(H, W, dtype=torch.bool)
    outside[win[0]:win[0] + win[2], win[1]:win[1] + win[3]] = False
    assert bool((got[:, outside] == 0).all()) and bool((got[:, ~outside] != 0).all())


def _close(g, g64, what, rtol=2e-5):
    err = (g.double() - g64).abs()
    band = rtol * (1.0 + g64.abs())
    assert bool((err <= band).all()), (what, float(err.max()), float(g64.abs().max()))


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("n", [2, 3])
def test_gradients_with_a_tile_sum_the_repeats(hw, n):
    H, W = hw
    for i, stages in enumerate(([("tile", n, n)], [("roll", 1, 2), ("tile", n, n), ("flip_h",), ("roll", -3, W + 5)],
                                [("flip_v",), ("tile", n, n), ("crop", 1, 0, n * H - 1, max(1, n * W - 2))])):
        got, want = _grad_pair(H, W, stages, 200 + i)
        _close(got, want, (hw, n, stages))
        if i == 0 and H * W > 100:                   # not vacuous: every texel really sums n^2 terms
            assert float(want.abs().max()) > 3.0


def test_fp16_and_batched_inputs_have_gradients():
    """fp16 maps: the result is fp16, so autograd hands the backward kernel an upstream gradient ROUNDED to fp16.  The weights here are
    fp16 values, so that cast is exact and the float64 reference sums the very terms the kernel sums.  Each source texel has two
    preimages: one fp32 addition (2^-24 of the sum), then one rounding of the sum to fp16 (2^-11 of it, 2^-25 absolute for a
    subnormal result) -- inside 2e-3 |g| + 1e-7."""
    from pypbr_amd import functional as F
    g = torch.Generator().manual_seed(12)
    x = (torch.rand(2, 3, 9, 14, generator=g) - 0.5).half().cuda().requires_grad_()
    out = F.remap_planes(x, (8, -1), (3, 1), negate=(1,), out_size=(18, 14))
    assert out.dtype == torch.float16
    w = torch.randn(out.shape, generator=g).half().float().cuda()
    (out.float() * w).sum().backward()
    x64 = x.detach().double().requires_grad_()
    rows = torch.tensor([(8 - i) % 9 for i in range(18)], device="cuda")
    cols = torch.tensor([(3 + j) % 14 for j in range(14)], device="cuda")
    ref = x64.index_select(2, rows).index_select(3, cols)
    ref = torch.cat([ref[:, :1], -ref[:, 1:2], ref[:, 2:]], dim=1)
    (ref * w.double()).sum().backward()
    assert x.grad.dtype == torch.float16
    err = (x.grad.double() - x64.grad).abs()
    print("\n[fp16 gradient] max |g - g64| %.3e, max |g64| %.3e" % (float(err.max()), float(x64.grad.abs().max())))
    assert bool((err <= 2e-3 * x64.grad.abs() + 1e-7).all())


# ---- through the renderer -------------------------------------------------------------------------------------------------------------
def _render_maps(seed, H, W):
    g = torch.Generator().manual_seed(seed)
    n = torch.cat([torch.rand(2, H, W, generator=g) - 0.5, torch.ones(1, H, W)], 0)
    return {"albedo": torch.rand(3, H, W, generator=g), "normal": n / n.norm(dim=0, keepdim=True),
            "roughness": torch.rand(1, H, W, generator=g) * 0.8 + 0.2, "metallic": torch.rand(1, H, W, generator=g)}


def test_rolled_and_flipped_material_renders_as_the_aten_transformed_maps():
    from pypbr_amd.models import CookTorranceBRDF
    maps = _render_maps(5, 45, 70)
    stages = [("roll", 3, 5), ("flip_h",), ("flip_v",)]
    mat = _material(maps)
    mat.roll((3, 5)).flip_horizontal().flip_vertical()
    other = _material({k: aten_stages(v, stages, k == "normal").contiguous() for k, v in maps.items()})
    brdf = CookTorranceBRDF(light_type="point")
    a = brdf(mat, LIGHT["view"], LIGHT["light"], LIGHT["intensity"], 1.0)
    b = brdf(other, LIGHT["view"], LIGHT["light"], LIGHT["intensity"], 1.0)
    assert a.shape == (3, 45, 70) and torch.equal(a, b)
    for k in maps:
        assert torch.equal(mat._maps[k], other._maps[k]), k


def test_rendering_loss_over_a_composed_material_fills_albedo_grad():
    from pypbr_amd import transforms as T
    from pypbr_amd.losses import RenderingLoss
    maps = _render_maps(6, 40, 64)
    target = _material(_render_maps(7, 48, 72))
    run = [T.RandomCrop(24, 36), T.RandomHorizontalFlip(), T.RandomVerticalFlip(), T.Roll((5, -7)), T.Tile(2)]
    grads = []
    for fuse in (True, False):
        mat = _material(maps, requires_grad=("albedo",))
        albedo = mat._raw["albedo"]
        random.seed(2)                                 # seed 2: both flips are drawn
        pred = T.Compose(run, fuse=fuse)(mat)
        assert pred.size == (48, 72)
        loss = RenderingLoss()(pred, target)
        loss.backward()
        assert albedo.grad is not None and albedo.grad.shape == (3, 40, 64) and float(albedo.grad.abs().max()) > 0
        grads.append(albedo.grad.detach().cpu())
    random.seed(2)
    draws = [random.random() for _ in range(4)]
    assert draws[2] < 0.5 and draws[3] < 0.5
    _close(grads[0], grads[1].double(), "fused against unfused")
    assert bool((grads[0] == 0).any())                # texels outside the crop window receive exactly nothing


# ---- Compose --------------------------------------------------------------------------------------------------------------------------
def test_compose_fused_equals_unfused_with_one_launch_per_block():
    """A run that folds into one index map is ONE launch for the material's nine planes.  Upstream's augmentation order puts the crop
    first: a roll behind a crop wraps inside the window, so that run is two maps and two launches."""
    from pypbr_amd import functional as F, transforms as T
    ins = _gold("in__37x53")
    foldable = [T.RandomHorizontalFlip(), T.RandomVerticalFlip(), T.Roll((3, -9)), T.Tile(2), T.RandomCrop(40, 64)]
    upstream_order = [T.RandomCrop(20, 32), T.RandomHorizontalFlip(), T.RandomVerticalFlip(), T.Roll((3, -9)), T.Tile(2)]
    for run, launches in ((foldable, 1), (upstream_order, 2)):
        for seed in range(6):
            mat = _material(ins)
            before = {k: (v, v.clone()) for k, v in mat._raw.items()}
            random.seed(seed)
            count = dict(F.LAUNCHES)
            fused = T.Compose(run)(mat)
            assert F.LAUNCHES["remap_planes"] - count["remap_planes"] == launches, (seed, launches)     # five stages, nine planes, one block
            assert F.LAUNCHES["remap_planes_backward"] == count["remap_planes_backward"]
            random.seed(seed)
            count = dict(F.LAUNCHES)
            unfused = T.Compose(run, fuse=False)(mat)
            assert F.LAUNCHES["remap_planes"] - count["remap_planes"] >= 2
            assert fused is not mat and fused.size == (40, 64) == unfused.size
            for k in G.MAPS:
                assert torch.equal(fused._maps[k], unfused._maps[k]), (seed, k)
                assert fused._maps[k].data_ptr() != mat._maps[k].data_ptr()
            for k, (same, copy) in before.items():         # the input material: the same tensors, the same values
                assert mat._raw[k] is same and torch.equal(same, copy), (seed, k)


def test_compose_splits_runs_at_other_callables_and_copies_what_it_does_not_move():
    from pypbr_amd import functional as F, transforms as T
    ins = _gold("in__37x53")
    mat = _material(ins)
    count = dict(F.LAUNCHES)
    out = T.Compose([T.FlipHorizontal(), T.Roll((1, 2)), T.InvertNormal(), T.FlipVertical(), T.Crop(3, 4, 10, 12)])(mat)
    assert F.LAUNCHES["remap_planes"] - count["remap_planes"] == 2
    plain = T.Compose([T.FlipHorizontal(), T.Roll((1, 2)), T.InvertNormal(), T.FlipVertical(), T.Crop(3, 4, 10, 12)], fuse=False)(mat)
    for k in G.MAPS:
        assert torch.equal(out._maps[k], plain._maps[k]), k
    same = T.Compose([T.FlipHorizontal(), T.Roll((37, 0)), T.FlipHorizontal()])(mat)          # folds to the identity: still a new material
    for k in G.MAPS:
        assert torch.equal(same._maps[k], mat._maps[k]) and same._maps[k].data_ptr() != mat._maps[k].data_ptr(), k


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------
GUARD_WIDTHS = (1, 3, 4, 5, 63, 65, 255, 257, 260)


@pytest.mark.parametrize("W", GUARD_WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guard_bands(W, dtype):
    from pypbr_amd import _native as N
    lib = N.lib()
    s = torch.cuda.current_stream().cuda_stream
    B, P, H = 2, 3, 5
    g = torch.Generator().manual_seed(W)
    x = (torch.rand(B, P, H, W, generator=g) - 0.5).to(dtype)
    code = N.F32 if dtype == torch.float32 else N.F16
    for (oy, sy, ox, sx, ho, wo) in ((0, 1, 0, 1, H, W), (H - 1, -1, W - 1, -1, H, W), (2, 1, (W + 5) % W, -1, 2 * H, 2 * W + 1),
                                     (1, -1, W // 2, 1, 3, max(1, W - 3))):
        G_ = Guards()
        xi, out = G_.input(x), G_.output((B, P, ho, wo), dtype)
        assert lib.pbr_remap_planes(xi.data_ptr(), P * H * W, H * W, out.data_ptr(), P * ho * wo, ho * wo, B, P, H, W, ho, wo, oy, sy, ox, sx, 2,
                                    code, s) == 0
        G_.check(("forward", W, dtype, oy, sy, ox, sx, ho, wo))
        rows = torch.tensor([(oy + sy * i) % H for i in range(ho)])
        cols = torch.tensor([(ox + sx * j) % W for j in range(wo)])
        want = x.index_select(2, rows).index_select(3, cols).clone()
        want[:, 1] = -want[:, 1]
        assert torch.equal(out.cpu(), want), (W, dtype, oy, sy, ox, sx, ho, wo)
        if dtype != torch.float32:
            continue
        G_ = Guards()
        go = torch.randn(B, P, ho, wo, generator=g)
        gi_, gs = G_.input(go), G_.output((B, P, H, W))
        assert lib.pbr_remap_planes_backward(gi_.data_ptr(), P * ho * wo, ho * wo, gs.data_ptr(), P * H * W, H * W, B, P, H, W, ho, wo, oy, sy,
                                             ox, sx, 2, s) == 0
        G_.check(("backward", W, oy, sy, ox, sx, ho, wo))
        x64 = x.double().requires_grad_()
        ref = x64.index_select(2, rows).index_select(3, cols)
        ref = torch.cat([ref[:, :1], -ref[:, 1:2], ref[:, 2:]], dim=1)
        (ref * go.double()).sum().backward()
        _close(gs.cpu(), x64.grad, ("backward", W, oy, sy, ox, sx, ho, wo))


# ---- offsets beyond 2^31 elements -----------------------------------------------------------------------------------------------------
def test_offsets_beyond_2_31_elements_are_right_in_the_last_image():
    """64-bit batch offsets: the last image starts past 2^31 elements in the source, the result and both gradients."""
    from pypbr_amd import _native as N, functional as F
    B, H, W = 180, 2048, 2048
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(B, 3, H, W, device="cuda", generator=g)
    assert x[B - 1].storage_offset() > 2 ** 31
    out = F.remap_planes(x, (5, -1), (2047, -1), negate=(1,))
    assert out[B - 1].storage_offset() > 2 ** 31
    last = F.remap_planes(x[B - 1], (5, -1), (2047, -1), negate=(1,))
    assert torch.equal(out[B - 1], last)
    assert float((last - out[0]).abs().max()) > 0.1                # not vacuous: the images differ
    want = torch.roll(x[B - 1].flip(-2), 6, dims=-2).flip(-1)
    want[1] = -want[1]
    assert torch.equal(last, want)
    del want
    gs = torch.empty_like(x)
    s = torch.cuda.current_stream().cuda_stream
    P = H * W
    assert N.lib().pbr_remap_planes_backward(out.data_ptr(), 3 * P, P, gs.data_ptr(), 3 * P, P, B, 3, H, W, H, W, 5, -1, 2047, -1, 2, s) == 0
    assert torch.equal(gs[B - 1], x[B - 1]) and torch.equal(gs[0], x[0])       # the adjoint of a signed permutation is its inverse
    del x, out, gs
    torch.cuda.empty_cache()


# ---- operators ------------------------------------------------------------------------------------------------------------------------
def test_opcheck_the_two_operators():
    from pypbr_amd import functional as F, torch_ops
    assert torch_ops.available()
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(4, 12, 21, generator=g) - 0.5).cuda().requires_grad_()
    go = torch.randn(4, 20, 30, generator=g).cuda()
    torch.library.opcheck(torch.ops.pbr_hip.remap_planes.default, (x, 3, -1, 20, 1, 5, 20, 30))
    torch.library.opcheck(torch.ops.pbr_hip.remap_planes_backward.default, (go, 12, 21, 3, -1, 20, 1, 5))
    x = x.detach().clone().requires_grad_()
    out = torch.ops.pbr_hip.remap_planes(x, 3, -1, 20, 1, 5, 20, 30)
    assert torch.equal(out, F.remap_planes(x.detach(), (3, -1), (20, 1), negate=(0, 2), out_size=(20, 30)))
    (out * go).sum().backward()
    y = x.detach().clone().requires_grad_()
    (F.remap_planes(y, (3, -1), (20, 1), negate=(0, 2), out_size=(20, 30)) * go).sum().backward()
    assert torch.equal(x.grad, y.grad)
