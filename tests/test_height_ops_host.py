"""Normal -> height on the host side (no GPU): the C ABI declares and exports the stages, argument errors come before any device work
with upstream's messages, the public names resolve, the launch counters gained no key, and the golden files are what
tools/gen_height_golden.py makes from the real reference."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("height_ops.npz", "height_ops_grad.npz")


def test_header_declares_and_library_exports_the_height_ops():
    from pypbr_amd import _native as N
    assert N.ABI_VERSION == 9 and "#define PBR_HIP_ABI_VERSION 9" in abi_header.RAW
    lib = N.lib()
    assert lib.pbr_abi_version() == 9


def test_workspace_is_one_partial_per_fixed_pixel_range():
    """24 bytes per 12288 pixels of every image: 512 x 512 has 22 partials, the last one ragged (4096 px) -- what the GPU suite's
    multi-workgroup case relies on; a shape beyond the reductions' 2^31 pixels has no workspace."""
    from pypbr_amd import _native as N
    lib = N.lib()
    assert lib.pbr_height_workspace_bytes(1, 1, 1) == 24
    assert lib.pbr_height_workspace_bytes(1, 96, 128) == 24 and lib.pbr_height_workspace_bytes(1, 96, 129) == 48
    assert lib.pbr_height_workspace_bytes(2, 512, 512) == 2 * 22 * 24 and (512 * 512) % 12288 == 4096
    assert lib.pbr_height_workspace_bytes(1, 65536, 32768) == 0 and lib.pbr_height_workspace_bytes(0, 4, 4) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """Null pointers, shapes, strides, alignment and dtypes return the ABI's codes without touching a device (there is none here)."""
    from pypbr_amd import _native as N
    lib = N.lib()
    a = 4096                                                     # never dereferenced: every call below is refused first
    assert lib.pbr_normal_divergence(None, 0, 0, a, 0, 1, 4, 4, 1.0, 0, N.F32, None) == N.ERR_NULL_MAP
    assert lib.pbr_normal_divergence(a, 48, 16, a, 16, 1, 0, 4, 1.0, 0, N.F32, None) == N.ERR_SHAPE
    assert lib.pbr_normal_divergence(a, -1, 16, a, 16, 1, 4, 4, 1.0, 0, N.F32, None) == N.ERR_SHAPE
    assert lib.pbr_normal_divergence(a, 48, 16, a, 16, 1, 4, 4, 1.0, 0, 7, None) == N.ERR_DTYPE
    assert lib.pbr_normal_divergence_backward(a, 48, 16, None, 16, a, 48, 16, 1, 4, 4, 1.0, 0, None) == N.ERR_NULL_MAP
    assert lib.pbr_normal_divergence_backward(a, 48, 16, a, 16, a, 48, -16, 1, 4, 4, 1.0, 0, None) == N.ERR_SHAPE
    assert lib.pbr_poisson_scale(None, 12, 1, 4, 4, None) == N.ERR_NULL_MAP
    assert lib.pbr_poisson_scale(a + 4, 12, 1, 4, 4, None) == N.ERR_SHAPE          # complex64 is 8-byte aligned
    assert lib.pbr_poisson_scale(a, 12, 1, 4, 0, None) == N.ERR_SHAPE
    assert lib.pbr_height_stats(a, 16, None, 1, 4, 4, None) == N.ERR_NULL_MAP
    assert lib.pbr_height_stats(a, 16, a, 1, 65536, 32768, None) == N.ERR_SHAPE
    assert lib.pbr_height_normalize(a, 16, a, a, 16, a, 1, 4, 4, 7, None) == N.ERR_DTYPE
    assert lib.pbr_height_normalize(a, 16, a, a, 16, None, 1, 4, 4, N.F32, None) == N.ERR_NULL_MAP
    assert lib.pbr_height_normalize_backward(a, 16, a, 16, a, a + 4, a, 16, 1, 4, 4, None) == N.ERR_SHAPE
    assert lib.pbr_height_normalize_backward(a, 16, a, 16, a, a, a, 16, -1, 4, 4, None) == N.ERR_SHAPE


def test_argument_errors_come_first_with_upstream_messages():
    from pypbr_amd import functional as F
    from pypbr_amd.materials import BasecolorMetallicMaterial
    with pytest.raises(ValueError, match=r"^Normal map is required to compute height\.$"):
        F.height_from_normal(None)
    with pytest.raises(ValueError, match=r"^Normal map must have three channels\.$"):
        F.height_from_normal(torch.rand(1, 8, 8))
    with pytest.raises(ValueError, match=r"^Normal map must have three channels\.$"):
        F.height_from_normal(torch.rand(2, 4, 8, 8))
    with pytest.raises(ValueError, match=r"^Unsupported normal convention\.$"):
        F.height_from_normal(torch.rand(3, 8, 8), 1.0, convention="sideways")
    with pytest.raises(TypeError, match="float32/float16"):
        F.height_from_normal(torch.rand(3, 8, 8).double())
    with pytest.raises(NotImplementedError, match="float32"):
        F.height_from_normal(torch.rand(3, 8, 8).half().requires_grad_())
    m = BasecolorMetallicMaterial(albedo=torch.rand(3, 8, 8), roughness=torch.rand(1, 8, 8), metallic=torch.rand(1, 8, 8))
    with pytest.raises(ValueError, match=r"^Normal map is required to compute height\.$"):
        m.compute_height_from_normal(2.0)
    m.normal_convention = "sideways"
    with pytest.raises(ValueError, match=r"^Unsupported normal convention\.$"):
        m.compute_height_from_normal(2.0)


def test_the_public_names_resolve():
    from pypbr_amd import _height_ops, compat, functional as F
    from pypbr_amd.materials import BasecolorMetallicMaterial, DiffuseSpecularMaterial, MaterialBase
    assert F.height_from_normal is _height_ops.height_from_normal and F._HeightFromNormalFn is _height_ops._HeightFromNormalFn
    for cls in (MaterialBase, BasecolorMetallicMaterial, DiffuseSpecularMaterial):
        assert callable(cls.compute_height_from_normal)
    compat.install(force=True)
    try:
        from pypbr.materials import MaterialBase as Aliased
        assert Aliased.compute_height_from_normal is MaterialBase.compute_height_from_normal
    finally:
        compat.uninstall()


def test_the_launch_counters_gained_no_key():
    from pypbr_amd import _height_ops, functional as F  # noqa: F401  (importing the family must not register a counter)
    assert set(F.LAUNCHES) == {"remap_planes", "remap_planes_backward", "plane_ops", "plane_ops_backward", "rotate_planes", "rotate_planes_backward"}


def test_golden_files_are_small_float_arrays():
    for name in FILES:
        path = os.path.join(ROOT, "tests", "golden", name)
        assert os.path.getsize(path) < 2 ** 20, name
        z = np.load(path)
        for k in z.files:
            assert z[k].dtype == (np.float64 if k.startswith("ref64__") else np.float32), (name, k)


def test_golden_files_are_what_the_reference_makes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_height_golden as G
    out = subprocess.run([sys.executable, "-W", "ignore", os.path.join(ROOT, "tools", "gen_height_golden.py"), str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    for name in FILES:
        committed = np.load(os.path.join(ROOT, "tests", "golden", name))
        version, threads = G.meta(committed)
        fresh = np.load(os.path.join(tmp_path, name))
        assert sorted(fresh.files) == sorted(committed.files)
        exact = version == torch.__version__ and threads == G.THREADS
        for k in committed.files:
            assert committed[k].dtype.kind == "f", k
            if exact:
                assert np.array_equal(fresh[k], committed[k], equal_nan=True), k
            elif k.startswith("g32__") or k.startswith("g64__"):            # gradients reach 50: relative, the GPU suite's form
                assert np.all(np.abs(fresh[k] - committed[k]) <= 1e-6 * (1 + np.abs(committed[k]))), k
            elif not k.startswith("meta_"):
                assert np.allclose(fresh[k], committed[k], rtol=0, atol=1e-7, equal_nan=True), k
