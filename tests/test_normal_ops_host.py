"""The normal-map operations on the host side (no GPU): the C ABI declares and exports them, the reference's names resolve through
compat, argument errors come before any device work with upstream's messages, and the golden file is what the real reference makes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_normal_ops():
    from pypbr_amd import _native as N
    assert N.ABI_VERSION == 9 and "#define PBR_HIP_ABI_VERSION 9" in abi_header.RAW
    lib = N.lib()
    assert lib.pbr_abi_version() == 9


def test_compat_resolves_the_reference_names():
    from pypbr_amd import compat
    compat.install(force=True)
    try:
        import pypbr.utils as U
        from pypbr.materials import BasecolorMetallicMaterial, MaterialBase
        for name in ("compute_normal_from_height", "rotate_normals", "invert_normal"):
            assert callable(getattr(U, name)), name
        for name in ("compute_normal_from_height", "adjust_normal_strength", "invert_normal"):
            assert callable(getattr(MaterialBase, name)) and callable(getattr(BasecolorMetallicMaterial, name)), name
        assert not hasattr(U, "compute_height_from_normal")
    finally:
        compat.uninstall()


def test_argument_errors_come_first_with_upstream_messages():
    from pypbr_amd import functional as F, utils
    from pypbr_amd.materials import BasecolorMetallicMaterial
    with pytest.raises(ValueError, match=r"^Height map is required to compute normals\.$"):
        utils.compute_normal_from_height(None)
    with pytest.raises(ValueError, match=r"^Unsupported normal convention\.$"):
        utils.compute_normal_from_height(torch.rand(1, 8, 8), 1.0, convention="sideways")
    with pytest.raises(ValueError, match="1 channel"):
        F.normal_from_height(torch.rand(3, 8, 8))
    with pytest.raises(ValueError, match="1 channel"):
        F.normal_from_height(torch.rand(2, 3, 8, 8))
    m = BasecolorMetallicMaterial(albedo=torch.rand(3, 8, 8), roughness=torch.rand(1, 8, 8), metallic=torch.rand(1, 8, 8))
    with pytest.raises(ValueError, match=r"^Height map is required to compute normals\.$"):
        m.compute_normal_from_height(2.0)
    m.height = torch.rand(3, 8, 8)
    with pytest.raises(ValueError, match="1 channel"):
        m.compute_normal_from_height(2.0)
    m.normal_convention = "sideways"
    with pytest.raises(ValueError, match=r"^Unsupported normal convention\.$"):
        m.compute_normal_from_height(2.0)


def test_invert_normal_without_a_normal_map_swaps_the_convention():
    from pypbr_amd.materials import BasecolorMetallicMaterial, NormalConvention
    m = BasecolorMetallicMaterial(albedo=torch.rand(3, 4, 4), roughness=torch.rand(1, 4, 4), metallic=torch.rand(1, 4, 4))
    assert m.normal_convention == NormalConvention.OPENGL
    assert m.invert_normal() is m and m.normal_convention == NormalConvention.DIRECTX
    assert m.invert_normal().normal_convention == NormalConvention.OPENGL
    assert m._maps.get("normal") is None


def test_golden_file_is_what_the_reference_makes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_normal_golden as G
    committed = np.load(os.path.join(ROOT, "tests", "golden", "normal_ops.npz"))
    version, threads = G.meta(committed)
    out = subprocess.run([sys.executable, "-W", "ignore", os.path.join(ROOT, "tools", "gen_normal_golden.py"), str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = np.load(os.path.join(tmp_path, "normal_ops.npz"))
    assert sorted(fresh.files) == sorted(committed.files)
    exact = version == torch.__version__ and threads == G.THREADS
    for k in committed.files:
        assert committed[k].dtype.kind == "f", k
        if exact:
            assert np.array_equal(fresh[k], committed[k], equal_nan=True), k
        elif not k.startswith("meta_"):
            assert np.allclose(fresh[k], committed[k], rtol=0, atol=1e-7, equal_nan=True), k
