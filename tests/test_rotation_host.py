"""Material rotation on the host side (no GPU): the C ABI declares and exports the two rotate entry points (ABI still 9), argument errors
come before the library is touched, the ATen restatement of upstream's chain (tools/rotate_oracle.py) reproduces the fixture the real
reference wrote, the closed-form index function of functional.rotate_plan / rotate_indices equals that restatement on every fixture case
and on the whole GPU test matrix, RandomRotate makes upstream's draw, and the host constants are the expected ones."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rotate_golden as G  # noqa: E402
import rotate_oracle as O  # noqa: E402

import abi_header  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402
from pypbr_amd import rotation as R  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "rotate.npz"))


def _in(size, k):
    return torch.from_numpy(GOLD["in__%s__%s" % (size, k)])


def _material(h=8, w=24):
    from pypbr_amd.materials import BasecolorMetallicMaterial
    return BasecolorMetallicMaterial(albedo=torch.rand(3, h, w), roughness=torch.rand(1, h, w), metallic=torch.rand(1, h, w))


def test_header_declares_and_library_exports_the_rotate_entry_points():
    from pypbr_amd import _native as N
    assert "pbr_rotate_geom" in abi_header.TEXT
    assert N.ABI_VERSION == 9 and "#define PBR_HIP_ABI_VERSION 9" in abi_header.RAW
    lib = N.lib()
    assert lib.pbr_abi_version() == 9


def test_the_upstream_names_stay_where_they_are():
    """The feature lives in pypbr_amd.rotation; transforms, its functional and MaterialBase neither import nor re-export it."""
    from pypbr_amd import transforms as T
    from pypbr_amd.materials import MaterialBase
    for name in R.__all__:
        assert callable(getattr(R, name)), name
        assert not hasattr(T, name) and not hasattr(T.functional, name) and not hasattr(MaterialBase, name), name
    for mod in ("transforms.py", "_transforms_functional.py", "materials.py"):
        assert "rotation" not in re.sub(r'""".*?"""', "", open(os.path.join(ROOT, "pypbr_amd", mod)).read(), flags=re.S), mod


def test_argument_errors_come_before_the_library_is_touched(monkeypatch):
    from pypbr_amd import _native as N

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(N, "lib", no_library)
    monkeypatch.setattr(N, "require_device", no_library)
    m = _material(8, 24)
    before = dict(m._raw)
    with pytest.raises(ValueError, match="padding mode"):
        R.rotate(m, 30.0, padding_mode="reflect")
    with pytest.raises(ValueError, match="circular"):
        R.rotate(m, 30.0, padding_mode="circular")                   # 8 x 24: pad 18 > 8, upstream's F.pad raises
    with pytest.raises(ValueError, match="padding mode"):
        R.Rotate(30.0, padding_mode="reflect")
    with pytest.raises(ValueError, match="padding mode"):
        R.RandomRotate(padding_mode="reflect")
    with pytest.raises(ValueError, match="circular"):
        R.Rotate(30.0, padding_mode="circular")(m)
    random.seed(3)
    first = random.random()
    random.seed(3)
    with pytest.raises(ValueError, match="padding mode"):
        R.random_rotate(m, padding_mode="reflect")
    assert random.random() == first                                   # a refused call draws nothing
    with pytest.raises(ValueError, match="padding mode"):
        F.rotate_maps(torch.rand(3, 8, 8), 10.0, padding_mode="reflect")
    with pytest.raises(ValueError, match="circular"):
        F.rotate_maps(torch.rand(3, 8, 24), 10.0, padding_mode="circular")
    with pytest.raises(ValueError, match="32 planes"):
        F.rotate_maps(torch.rand(33, 8, 8), 10.0)
    with pytest.raises(ValueError, match="normal_first_plane"):
        F.rotate_maps(torch.rand(4, 8, 8), 10.0, normal_first_plane=2)
    with pytest.raises(TypeError):
        F.rotate_maps(torch.rand(3, 8, 8).double(), 10.0)
    with pytest.raises(ValueError):
        F.rotate_maps(torch.rand(8, 8), 10.0)
    assert all(m._raw[k] is v and v.device.type == "cpu" for k, v in before.items())       # nothing moved, nothing replaced


def test_upstreams_f_pad_raises_where_this_package_does():
    with pytest.raises(RuntimeError):
        O.rotate_map(torch.rand(1, 8, 24), 30.0, False, "circular")


# ---- the host constants ---------------------------------------------------------------------------------------------------------------
CONSTANTS = {
    # (h, w, angle, expand, mode): (H, W, pad, oh, ow, top, left)
    (64, 64, 180.0, True, "constant"): (65, 65, 27, 118, 118, 26, 26),           # upstream's quirk: 64 * |cos pi| + 64 * |sin pi| > 64
    (64, 64, 0.0, False, "constant"): (64, 64, 27, 118, 118, 27, 27),
    (13, 9, 90.0, False, "constant"): (13, 9, 3, 15, 19, 1, 5),
    (13, 9, 90.0, True, "constant"): (9, 13, 7, 23, 27, 7, 7),
    (16, 24, 33.3, False, "circular"): (16, 24, 13, 64, 66, 24, 21),
    (8, 8, 45.0, False, "constant"): (8, 8, 4, 24, 24, 8, 8),
}


@pytest.mark.parametrize("case", sorted(CONSTANTS, key=str))
def test_host_constants(case):
    """Against hand-checkable values and, for (oh, ow), against the size of what the restated torchvision rotate returns."""
    h, w, angle, expand, mode = case
    p = F.rotate_plan(*case)
    assert F.rotate_plan(*case) is p                                   # kept per (h, w, angle, expand, mode)
    H, W = O.target_size(h, w, angle, expand)
    pad = int(np.ceil(np.sqrt(H * H + W * W))) - H
    assert (p.H, p.W, p.pad, p.Hp, p.Wp) == (H, W, pad, h + 2 * pad, w + 2 * pad)
    rotated = O.rotate(torch.zeros(1, p.Hp, p.Wp), angle, expand=True)
    assert tuple(rotated.shape[-2:]) == (p.oh, p.ow)
    assert (p.top, p.left) == (int(round((p.oh - H) / 2.0)), int(round((p.ow - W) / 2.0)))
    assert (p.H, p.W, p.pad, p.oh, p.ow, p.top, p.left) == CONSTANTS[case]
    assert p.x0 == p.left - p.ow / 2 + 0.5 and p.y0 == p.top - p.oh / 2 + 0.5


# ---- the closed form against the restated chain ---------------------------------------------------------------------------------------
def _gather(t, idx):
    """t (C,h,w) through an (H,W) index map of source offsets, -1 = 0."""
    flat = torch.cat([t.reshape(t.shape[0], -1), torch.zeros(t.shape[0], 1, dtype=t.dtype)], dim=1)
    return flat[:, torch.where(idx < 0, torch.full_like(idx, flat.shape[1] - 1), idx)]


def test_closed_form_equals_the_restated_chain_on_the_whole_matrix():
    """An index image (texel k holds k + 1, fill is 0) through the ATen chain against rotate_indices: the same texel for EVERY pixel of
    every case the GPU tests run, strict and tie angles alike (the host's ATen and the closed form round alike here: the issue's check)."""
    n = 0
    for h, w, angle, expand, mode, strict in G.matrix():
        image = torch.arange(h * w, dtype=torch.float32).reshape(1, h, w) + 1
        want = O.rotate_map(image, angle, expand, mode)[0]
        plan = F.rotate_plan(h, w, angle, expand, mode)
        got = (F.rotate_indices(plan) + 1).float()
        assert got.shape == want.shape == (plan.H, plan.W) and torch.equal(got, want), (h, w, angle, expand, mode, int((got != want).sum()))
        n += 1
    assert n >= 150, n


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_oracle_and_closed_form_reproduce_the_golden_file(name):
    h, w, angle, expand, mode = G.CASES[name]
    size = "%dx%d" % (h, w)
    idx = F.rotate_indices(F.rotate_plan(h, w, angle, expand, mode))
    for k in G.MAPS:
        want = torch.from_numpy(GOLD["out__%s__%s" % (name, k)])
        oracle = O.rotate_material_map(k, _in(size, k), angle, expand, mode)
        if k == "normal":                                             # the same ATen calls as the reference's: equal bits on the torch build
            exact = G.meta(GOLD) == (torch.__version__, G.THREADS)    # and thread count that wrote the file, 1e-6 (the normal operations' bound) elsewhere
            torch.set_num_threads(G.THREADS)
            oracle = O.rotate_material_map(k, _in(size, k), angle, expand, mode)
            assert torch.equal(oracle, want) if exact else float((oracle - want).abs().max()) <= 1e-6, (name, k)
            moved = O.rotate_normals(_gather(_in(size, k), idx), angle)
            assert float((moved - want).abs().max()) <= 1e-6, (name, k)
        else:
            assert torch.equal(oracle, want), (name, k)
            assert torch.equal(_gather(_in(size, k), idx), want), (name, k)
    bx, by = G.band(F.rotate_plan(h, w, angle, expand, mode))
    assert torch.equal((bx | by).float(), torch.from_numpy(GOLD["band__" + name]))


def test_band_caps_hold_for_every_case():
    strict, tie = G.check_band_caps()
    print("\n[tie band] largest share: strict %.4f, tie %.4f" % (strict, tie))
    assert strict <= G.STRICT_CAP and tie <= G.TIE_CAP
    assert tie > 0.02                                                 # the tie angles do put pixels on ties


def test_candidates_contain_the_closed_form_everywhere():
    for h, w, angle, expand, mode, strict in G.matrix():
        plan = F.rotate_plan(h, w, angle, expand, mode)
        idx, cands = F.rotate_indices(plan), G.candidates(plan)
        ok = torch.zeros_like(idx, dtype=torch.bool)
        for c in cands:
            ok |= c == idx
        assert bool(ok.all()), (h, w, angle, expand, mode)


@pytest.mark.parametrize("seed", G.SEEDS)
def test_random_rotate_makes_upstreams_draw(seed):
    want = float(GOLD["random__%d" % seed][0])
    random.seed(seed)
    assert R.random_angle(*G.RANDOM_RANGE) == want
    after = random.random()
    random.seed(seed)
    random.random()
    assert random.random() == after                                   # one draw: the stream is where upstream leaves it
    h, w = G.RANDOM_SIZE
    idx = F.rotate_indices(F.rotate_plan(h, w, want, False, "constant"))
    for k in ("albedo", "roughness"):
        assert torch.equal(_gather(_in("%dx%d" % (h, w), k), idx), torch.from_numpy(GOLD["out__random%d__%s" % (seed, k)])), (seed, k)


def test_golden_file_is_what_the_reference_makes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    version, threads = G.meta(GOLD)
    out = subprocess.run([sys.executable, "-W", "ignore", os.path.join(ROOT, "tools", "gen_rotate_golden.py"), str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = np.load(os.path.join(tmp_path, "rotate.npz"))
    assert sorted(fresh.files) == sorted(GOLD.files)
    exact = version == torch.__version__ and threads == G.THREADS
    for k in GOLD.files:
        assert GOLD[k].dtype.kind == "f", k
        if exact:
            assert np.array_equal(fresh[k], GOLD[k], equal_nan=True), k
        elif not k.startswith("meta_"):
            assert np.allclose(fresh[k], GOLD[k], rtol=0, atol=1e-7, equal_nan=True), k
