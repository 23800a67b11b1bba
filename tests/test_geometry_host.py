"""The geometric material transforms on the host side (no GPU): the C ABI declares and exports the two remap entry points (ABI still 9),
the reference's `pypbr.transforms` names resolve through compat (and the rotate family does not), crop errors come before any device work,
the host-side folding of chains into index maps equals step-by-step flip / roll / slice / repeat, the random transforms make upstream's
draws after random.seed, and the golden file is what the real reference makes."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_geometry_golden as G  # noqa: E402

import abi_header  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402
from pypbr_amd import transforms as T  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "geometry.npz"))


def test_header_declares_and_library_exports_the_remap_entry_points():
    from pypbr_amd import _native as N
    assert N.ABI_VERSION == 9 and "#define PBR_HIP_ABI_VERSION 9" in abi_header.RAW
    lib = N.lib()
    assert lib.pbr_abi_version() == 9


def test_compat_resolves_transforms_and_has_no_rotate():
    from pypbr_amd import compat
    compat.install(force=True)
    try:
        import pypbr.transforms
        import pypbr.transforms.functional as TF
        from pypbr.transforms import Compose
        from pypbr.transforms.functional import roll
        from pypbr.materials import MaterialBase
        assert Compose is T.Compose and roll is T.functional.roll and pypbr.transforms.functional is TF
        for name in ("Compose", "Resize", "RandomResize", "Crop", "CenterCrop", "RandomCrop", "Tile", "FlipHorizontal", "FlipVertical",
                     "RandomHorizontalFlip", "RandomVerticalFlip", "Roll", "InvertNormal", "AdjustNormalStrength", "ToLinear", "ToSrgb"):
            assert callable(getattr(pypbr.transforms, name)), name
        for name in ("resize", "random_resize", "crop", "center_crop", "random_crop", "tile", "flip_horizontal", "flip_vertical",
                     "random_horizontal_flip", "random_vertical_flip", "roll", "invert_normal_map", "adjust_normal_strength", "to_linear",
                     "to_srgb"):
            assert callable(getattr(TF, name)), name
        for name in ("crop", "flip_horizontal", "flip_vertical", "roll"):
            assert callable(getattr(MaterialBase, name)), name
        for name in ("Rotate", "RandomRotate"):
            assert not hasattr(pypbr.transforms, name), name
        for name in ("rotate", "random_rotate"):
            assert not hasattr(TF, name) and not hasattr(MaterialBase, name), name
    finally:
        compat.uninstall()


def _material(h=8, w=10):
    from pypbr_amd.materials import BasecolorMetallicMaterial
    return BasecolorMetallicMaterial(albedo=torch.rand(3, h, w), roughness=torch.rand(1, h, w), metallic=torch.rand(1, h, w))


@pytest.mark.parametrize("window", [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (5, 0, 4, 4), (0, 7, 4, 4), (0, 0, 9, 4), (0, 0, 4, 11)])
def test_crop_errors_come_before_any_device_work(window):
    m = _material()
    before = {k: v for k, v in m._raw.items()}
    with pytest.raises(ValueError, match="crop"):
        m.crop(*window)
    with pytest.raises(ValueError, match="crop"):
        T.functional.crop(m, *window)
    with pytest.raises(ValueError, match="crop"):
        T.Compose([T.FlipHorizontal(), T.Crop(*window)])(m)
    assert all(m._raw[k] is v and v.device.type == "cpu" for k, v in before.items())       # nothing moved, nothing replaced


def test_remap_planes_argument_errors_come_first():
    t = torch.rand(3, 4, 5)
    for kw in (dict(ymap=(4, 1), xmap=(0, 1)), dict(ymap=(0, 1), xmap=(5, 1)), dict(ymap=(-1, 1), xmap=(0, 1)), dict(ymap=(0, 0), xmap=(0, 1)),
               dict(ymap=(0, 1), xmap=(0, 2)), dict(ymap=(0, 1), xmap=(0, 1), out_size=(0, 5)), dict(ymap=(0, 1), xmap=(0, 1), negate=(3,))):
        with pytest.raises(ValueError):
            F.remap_planes(t, **kw)
    with pytest.raises(ValueError, match="32 planes"):
        F.remap_planes(torch.rand(33, 4, 5), (0, 1), (0, 1))
    with pytest.raises(TypeError):
        F.remap_planes(t.double(), (0, 1), (0, 1))
    with pytest.raises(ValueError):
        F.remap_planes(torch.rand(4, 5), (0, 1), (0, 1))


# ---- folding --------------------------------------------------------------------------------------------------------------------------
def step_by_step(t, stages):
    """The stages as the reference's methods run them on a (C,H,W) tensor: flip / roll / slicing / repeat (base.py:506-537, :605-655),
    the signs of a normal map's planes 0 / 1 included when `t` has 3 planes named so by the caller."""
    for st in stages:
        if st[0] == "flip_h":
            t = t.flip(-1)
        elif st[0] == "flip_v":
            t = t.flip(-2)
        elif st[0] == "crop":
            top, left, h, w = st[1:]
            t = t[..., top:top + h, left:left + w]
        elif st[0] == "roll":
            t = torch.roll(t, (st[1], st[2]), dims=(-2, -1))
        elif st[0] == "tile":
            t = t.repeat(1, st[1], st[2])
    return t


def apply_maps(t, chain, normal=False):
    """PlaneMaps applied one after the other by plain indexing (what the kernel does on the device)."""
    for pm in chain:
        rows, cols = pm.indices()
        t = t[:, rows][:, :, cols]
        if normal:
            t = t.clone()
            for p in (0, 1):
                if pm.neg[p]:
                    t[p] = -t[p]
    return t


def random_chain(rng, h, w):
    stages = []
    for _ in range(rng.randint(1, 5)):
        kind = rng.choice(("flip_h", "flip_v", "crop", "roll", "tile"))
        if kind == "crop":
            ch, cw = rng.randint(1, h), rng.randint(1, w)
            stages.append(("crop", rng.randint(0, h - ch), rng.randint(0, w - cw), ch, cw))
            h, w = ch, cw
        elif kind == "roll":
            stages.append(("roll", rng.randint(-2 * h, 2 * h), rng.randint(-2 * w, 2 * w)))
        elif kind == "tile":
            n = rng.randint(1, 3)
            if h * n > 40 or w * n > 40:
                continue
            stages.append(("tile", n, n))
            h, w = h * n, w * n
        else:
            stages.append((kind,))
    return stages or [("flip_h",)]


def test_folded_chains_equal_step_by_step():
    rng = random.Random(20261017)
    chains, single, moved = 3000, 0, 0
    for i in range(chains):
        h, w = rng.randint(1, 9), rng.randint(1, 9)
        stages = random_chain(rng, h, w)
        maps = F.fold_stages(h, w, stages)
        t = torch.arange(h * w, dtype=torch.float32).reshape(1, h, w)
        want = step_by_step(t, stages)
        got = apply_maps(t, maps)
        assert got.shape == want.shape and torch.equal(got, want), (i, h, w, stages)
        if maps:
            assert maps[-1].size == tuple(want.shape[-2:])
        # the signs: a normal map's plane 0 flips with every horizontal flip, plane 1 with every vertical one
        signs = [sum(1 for st in stages if st[0] == k) % 2 == 1 for k in ("flip_h", "flip_v")]
        assert [sum(1 for pm in maps if pm.neg[p]) % 2 == 1 for p in (0, 1)] == signs, (i, stages)
        single += len(maps) <= 1
        moved += len(maps) >= 1
    # not by materialising every stage: most chains are ONE map (the model check behind DESIGN.md 3.9 gives about 80 %)
    assert single >= chains // 2, (single, chains)
    assert moved >= chains // 2, (moved, chains)
    print("\n[folding] %d of %d random chains fold into one index map" % (single, chains))


def test_folding_rules_one_by_one():
    pm = F.PlaneMap(5, 7)
    assert pm.identity and pm.indices() == (list(range(5)), list(range(7)))
    assert pm.flip(True) and pm.xmap == (6, -1) and pm.neg == [True, False]
    assert pm.crop(1, 2, 3, 4) and pm.size == (3, 4) and pm.ymap == (1, 1) and pm.xmap == (4, -1)
    assert not pm.roll(1, 0) and not pm.roll(0, 1) and not pm.tile(2, 2)        # 3 % 5, 4 % 7: materialise first
    assert pm.roll(3, 8) and pm.roll(0, 0) and pm.tile(1, 1)                    # whole turns and tile(1) move nothing
    assert pm.size == (3, 4) and pm.ymap == (1, 1) and pm.xmap == (4, -1)
    full = F.PlaneMap(5, 7)
    assert full.roll(-6, 9) and full.ymap == (1, 1) and full.xmap == (5, 1)
    assert full.tile(2, 3) and full.size == (10, 21) and full.roll(7, 0) and full.ymap == (4, 1)
    with pytest.raises(ValueError):
        full.tile(0, 1)
    with pytest.raises(ValueError, match="crop"):
        full.crop(0, 0, 11, 1)
    assert F.fold_stages(4, 4, [("flip_h",), ("flip_h",), ("roll", 4, -8)]) == []
    assert len(F.fold_stages(37, 53, [("crop", 0, 0, 7, 9), ("roll", 3, 4)])) == 2


# ---- the random transforms make upstream's draws --------------------------------------------------------------------------------------
def _gold(prefix):
    return {k: torch.from_numpy(GOLD["%s__%s" % (prefix, k)]) for k in G.MAPS}


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_transforms_make_upstreams_draws(seed):
    """The stages this package resolves after random.seed(k), applied by plain indexing on the host, give the maps the reference's
    RandomCrop / RandomHorizontalFlip / RandomVerticalFlip left in the fixture after the same seed."""
    run = [T.RandomCrop(*G.RANDOM_CROP), T.RandomHorizontalFlip(), T.RandomVerticalFlip()]
    random.seed(seed)
    stages = T.Compose._resolve((37, 53), run)
    assert stages[0][0] == "crop" and stages[0][3:] == G.RANDOM_CROP
    after = random.random()
    random.seed(seed)
    for _ in range(4):                   # top, left, one draw per flip: the stream is where upstream leaves it
        random.random()
    assert random.random() == after
    maps = F.fold_stages(37, 53, stages)
    ins, outs = _gold("in__37x53"), _gold("out__37x53__random%d" % seed)
    for k in G.MAPS:
        assert torch.equal(apply_maps(ins[k], maps, normal=(k == "normal")), outs[k]), (seed, k, stages)
    # the functional forms draw the same window, in the same order
    random.seed(seed)
    assert T.functional.random_crop_window((37, 53), G.RANDOM_CROP) == stages[0][1:]


def test_random_resize_draws_height_first():
    random.seed(5)
    a, b = random.random(), random.random()
    random.seed(5)
    assert T.functional.random_resize_size(10, 50) == (int(10 + 40 * a), int(10 + 40 * b))


def test_every_fixture_case_is_its_stages_by_plain_indexing():
    """The fixture against the host model: every recorded case equals its stages folded and applied by indexing (so a failure of the GPU
    golden test is the kernel's, not the model's)."""
    for case, (m, stages) in G.CASES.items():
        if stages[0][0] == "random":
            continue
        ins, outs = _gold("in__" + m), _gold("out__" + case)
        for k in G.MAPS:
            h, w = ins[k].shape[-2:]
            assert torch.equal(apply_maps(ins[k], F.fold_stages(h, w, stages), normal=(k == "normal")), outs[k]), (case, k)


def test_golden_file_is_what_the_reference_makes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    version, threads = G.meta(GOLD)
    out = subprocess.run([sys.executable, "-W", "ignore", os.path.join(ROOT, "tools", "gen_geometry_golden.py"), str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = np.load(os.path.join(tmp_path, "geometry.npz"))
    assert sorted(fresh.files) == sorted(GOLD.files)
    exact = version == torch.__version__ and threads == G.THREADS
    for k in GOLD.files:
        assert GOLD[k].dtype.kind == "f", k
        if exact:
            assert np.array_equal(fresh[k], GOLD[k], equal_nan=True), k
        elif not k.startswith("meta_"):
            assert np.allclose(fresh[k], GOLD[k], rtol=0, atol=1e-7, equal_nan=True), k
