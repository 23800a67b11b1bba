"""Packed material tensors on the host side (no GPU): the C ABI declares and exports pbr_plane_ops and its gradient (ABI still 9), the
reference's names resolve through compat, every argument error of MaterialBase.as_tensor / from_tensor carries upstream's type and message
and comes before any device work, pbr_plane_ops returns its caller-error codes without a device, and the golden file is what the real
reference makes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_packing_golden as G  # noqa: E402

import abi_header  # noqa: E402
from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402
from pypbr_amd.materials import BasecolorMetallicMaterial, DiffuseSpecularMaterial, MaterialBase  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "packing.npz"))


def test_header_declares_and_library_exports_the_plane_op_entry_points():
    raw, text = abi_header.RAW, abi_header.TEXT
    assert "pbr_plane_op;" in text and "#define PBR_MAX_PLANE_OPS 32" in raw and N.MAX_PLANE_OPS == 32
    assert N.ABI_VERSION == 9 and "#define PBR_HIP_ABI_VERSION 9" in raw
    lib = N.lib()
    assert lib.pbr_abi_version() == 9
    assert ctypes.sizeof(N.PlaneOp) == 88                        # 2 x int32, 3 x (pointer, 2 x int64), 2 x float


def test_compat_resolves_the_packing_names():
    from pypbr_amd import compat
    compat.install(force=True)
    try:
        from pypbr.materials import MaterialBase as M
        assert M is MaterialBase
        assert callable(M.as_tensor) and callable(M.from_tensor) and isinstance(M.normal_rgb, property)
        for cls in (BasecolorMetallicMaterial, DiffuseSpecularMaterial):
            assert cls.from_tensor.__func__ is MaterialBase.from_tensor.__func__ and cls.as_tensor is MaterialBase.as_tensor
    finally:
        compat.uninstall()


def _material(h=4, w=5):
    return BasecolorMetallicMaterial(albedo=torch.rand(3, h, w), roughness=torch.rand(1, h, w), metallic=torch.rand(1, h, w))


@pytest.mark.parametrize("names, exc, message", [
    ("albedo", TypeError, "names must be a list of strings or tuples."),
    (("albedo",), TypeError, "names must be a list of strings or tuples."),
    ([("albedo", 1, 2)], ValueError, "Each tuple in names must have exactly two elements: (map_name, channel_limit)."),
    ([(3, 1)], TypeError, "The first element of each tuple must be a string (map name)."),
    ([("albedo", 0)], ValueError, "The second element of each tuple must be a positive integer (channel limit)."),
    ([("albedo", -2)], ValueError, "The second element of each tuple must be a positive integer (channel limit)."),
    ([("albedo", 1.0)], ValueError, "The second element of each tuple must be a positive integer (channel limit)."),
    ([3], TypeError, "Each item in names must be either a string or a tuple of (str, int)."),
    ([["albedo", 1]], TypeError, "Each item in names must be either a string or a tuple of (str, int)."),
    (["height"], KeyError, "Map 'height' does not exist in the texture maps."),
    (["albedo", ("normal", 2)], KeyError, "Map 'normal' does not exist in the texture maps."),
    ([("albedo", 4)], ValueError, "Requested 4 channels for map 'albedo', but only 3 channels are available."),
    ([("roughness", 2)], ValueError, "Requested 2 channels for map 'roughness', but only 1 channels are available."),
])
def test_as_tensor_argument_errors_are_upstreams_and_come_first(names, exc, message):
    m = _material()
    before = dict(m._raw)
    with pytest.raises(exc) as e:
        m.as_tensor(names=names)
    assert (e.value.args[0] if exc is KeyError else str(e.value)) == message
    assert all(m._raw[k] is v and v.device.type == "cpu" for k, v in before.items())       # nothing moved, nothing replaced


def test_as_tensor_errors_that_depend_on_the_maps():
    with pytest.raises(ValueError) as e:
        MaterialBase().as_tensor()
    assert str(e.value) == "No valid texture maps found to stack."
    m = _material()
    m._raw["height"] = torch.rand(1, 3, 5)
    with pytest.raises(ValueError) as e:
        m.as_tensor()
    assert str(e.value) == "All texture maps must have the same spatial dimensions for concatenation."
    with pytest.raises(ValueError) as e:
        m.as_tensor(names=["height", "albedo"], normalize=True)
    assert str(e.value) == "All texture maps must have the same spatial dimensions for concatenation."
    m._raw["height"] = None
    with pytest.raises(TypeError) as e:
        m.as_tensor()
    assert str(e.value) == "Map 'height' is not a torch.Tensor."


@pytest.mark.parametrize("cls", [MaterialBase, BasecolorMetallicMaterial, DiffuseSpecularMaterial])
@pytest.mark.parametrize("names, exc, message", [
    (None, ValueError, "Packed tensor has 4 channels, but configuration expects 0 channels."),
    ([], ValueError, "Packed tensor has 4 channels, but configuration expects 0 channels."),
    (["albedo"], KeyError, "Cannot infer channel count for map 'albedo'. Provide a tuple instead."),
    ([("albedo", 3), "roughness"], KeyError, "Cannot infer channel count for map 'roughness'. Provide a tuple instead."),
    ([("albedo", 3, 1)], ValueError, "Each tuple must be (map_name, channel_limit)."),
    ([("albedo",)], ValueError, "Each tuple must be (map_name, channel_limit)."),
    ([["albedo", 4]], TypeError, "Configuration items must be a string or tuple (str, int)."),
    ([4], TypeError, "Configuration items must be a string or tuple (str, int)."),
    ([("albedo", 3)], ValueError, "Packed tensor has 4 channels, but configuration expects 3 channels."),
    ([("albedo", 3), ("normal", 2)], ValueError, "Packed tensor has 4 channels, but configuration expects 5 channels."),
])
def test_from_tensor_argument_errors_are_upstreams_and_come_first(cls, names, exc, message):
    with pytest.raises(exc) as e:
        cls.from_tensor(torch.rand(4, 3, 5), names=names)
    assert (e.value.args[0] if exc is KeyError else str(e.value)) == message


def test_from_tensor_other_argument_errors_need_no_device():
    with pytest.raises(ValueError):
        MaterialBase.from_tensor(torch.rand(3, 5), names=[("albedo", 3)])
    with pytest.raises(TypeError):
        MaterialBase.from_tensor(torch.rand(3, 3, 5).double(), names=[("albedo", 3)])
    with pytest.raises(ValueError):
        MaterialBase.from_tensor(torch.rand(3, 3, 5), names=[("albedo", 4), ("normal", -1)])
    empty = DiffuseSpecularMaterial.from_tensor(torch.rand(0, 3, 5))          # upstream: an empty configuration and no channels
    assert type(empty) is DiffuseSpecularMaterial and empty._raw == {}
    assert MaterialBase().normal_rgb is None


def test_functional_argument_errors_need_no_device():
    t = torch.rand(5, 3, 4)
    with pytest.raises(ValueError, match="configuration expects 4"):
        F.unpack_planes(t, [("albedo", 3), ("roughness", 1)])
    with pytest.raises(ValueError):
        F.unpack_planes(t, [("albedo", 5), ("roughness", 0)])
    with pytest.raises(ValueError):
        F.unpack_planes(torch.rand(3, 4), [("albedo", 3)])
    with pytest.raises(TypeError):
        F.unpack_planes(t.double(), [("albedo", 5)])
    with pytest.raises(ValueError, match="No valid texture maps"):
        F.pack_planes([])
    with pytest.raises(ValueError, match="same spatial dimensions"):
        F.pack_planes([torch.rand(1, 3, 4), torch.rand(1, 4, 3)])
    with pytest.raises(ValueError):
        F.pack_planes([torch.rand(1, 3, 4)], limits=[2])
    with pytest.raises(TypeError):
        F.pack_planes([torch.rand(1, 3, 4), torch.rand(1, 3, 4).half()])
    with pytest.raises(ValueError):
        F.pack_planes([torch.rand(1, 3, 4)], limits=[None, None])


def _op(kind=N.PLANE_AFFINE, src=0x10000, dst=0x20000, ps=64, **kw):
    o = N.PlaneOp(kind, 0, src, 0, ps, dst, 0, ps, None, 0, 0, 1.0, 0.0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_plane_ops_caller_errors_come_back_without_a_device():
    """Every check runs before anything is launched: the pointers are never dereferenced."""
    lib = N.lib()

    def call(ops, n=None, batch=1, pixels=64, dtype=N.F32, fn=lib.pbr_plane_ops):
        table = (N.PlaneOp * max(1, len(ops)))(*ops)
        return fn(table, len(ops) if n is None else n, batch, pixels, dtype, None)
    bwd = lib.pbr_plane_ops_backward
    assert lib.pbr_plane_ops(None, 1, 1, 64, N.F32, None) == N.ERR_NULL_MAP
    assert bwd(None, 1, 1, 64, N.F32, None) == N.ERR_NULL_MAP
    assert call([_op()], n=0) == N.ERR_SHAPE and call([_op()], n=33) == N.ERR_SHAPE and call([_op()], n=-1) == N.ERR_SHAPE
    assert call([_op()], batch=0) == N.ERR_SHAPE and call([_op()], pixels=0) == N.ERR_SHAPE and call([_op()], batch=65536) == N.ERR_SHAPE
    assert call([_op()], dtype=7) == N.ERR_DTYPE
    assert call([_op()], dtype=N.F16, fn=bwd) == N.ERR_DTYPE                     # gradients are fp32
    assert call([_op(kind=2)]) == N.ERR_UNSUPPORTED and call([_op(), _op(kind=-1, dst=0x30000)]) == N.ERR_UNSUPPORTED
    assert call([_op(src=None)]) == N.ERR_NULL_MAP and call([_op(dst=None)]) == N.ERR_NULL_MAP
    assert call([_op(dst=None)], fn=bwd) == N.ERR_NULL_MAP
    assert call([_op(kind=N.PLANE_NORMAL_XY)], fn=bwd) == N.ERR_NULL_MAP         # the backward of NORMAL_XY needs the forward's input
    assert call([_op(src_batch_stride=-1)]) == N.ERR_SHAPE and call([_op(dst_plane_stride=-1)]) == N.ERR_SHAPE
    assert call([_op()], batch=2) == N.ERR_SHAPE                                  # two images written on top of each other
    assert call([_op(kind=N.PLANE_NORMAL_XY, dst_plane_stride=0)]) == N.ERR_SHAPE  # three planes written on top of each other
    assert call([_op(src=0x10002)]) == N.ERR_SHAPE and call([_op(dst=0x20001)], dtype=N.F16) == N.ERR_SHAPE     # not element-aligned
    # overlap: a destination inside a source, its own or another operation's; NORMAL_XY writes three planes
    assert call([_op(dst=0x10000 + 4 * 63)]) == N.ERR_SHAPE
    assert call([_op(), _op(src=0x40000, dst=0x10000)]) == N.ERR_SHAPE
    assert call([_op(kind=N.PLANE_NORMAL_XY, src=0x20000 + 4 * 2 * 64 + 4 * 10, dst=0x20000)]) == N.ERR_SHAPE
    assert call([_op(src=0x40000, dst=0x20000), _op(kind=N.PLANE_NORMAL_XY, src=0x30000, dst=0x50000, input=0x20000,
                                                   input_plane_stride=64)], fn=bwd) == N.ERR_SHAPE


def test_golden_file_is_what_the_reference_makes(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    version, threads = G.meta(GOLD)
    out = subprocess.run([sys.executable, "-W", "ignore", os.path.join(ROOT, "tools", "gen_packing_golden.py"), str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = np.load(os.path.join(tmp_path, "packing.npz"))
    assert sorted(fresh.files) == sorted(GOLD.files)
    exact = version == torch.__version__ and threads == G.THREADS
    for k in GOLD.files:
        assert GOLD[k].dtype.kind == "f", k
        if exact:
            assert np.array_equal(fresh[k], GOLD[k], equal_nan=True), k
        elif not k.startswith("meta_") and not k.startswith(("g32__", "g64__")):
            assert np.allclose(fresh[k], GOLD[k], rtol=0, atol=1e-7, equal_nan=True), k


def test_golden_file_holds_what_the_gpu_tests_need():
    """The near-circle set straddles the clamp inside its band, the gradient inputs keep their distance and hold clamped and unclamped
    pairs, the restatement bound the generator asserted is recorded, and the file fits the size limit of a committed file."""
    s = ((GOLD["nc_in"].astype(np.float64) * 2 - 1) ** 2).sum(0)
    assert (np.abs(1 - s) < 1.01 * G.NEAR_BAND).all() and (1 - s < 1e-6).any() and (1 - s >= 1e-6).any()
    for layout in G.GRAD_LAYOUTS:
        names = G.LAYOUTS[layout][1]
        c = sum(k for _, k in names[:[n for n, _ in names].index("normal")])
        s = ((GOLD["g_in__" + layout][c:c + 2].astype(np.float64) * 2 - 1) ** 2).sum(0)
        assert (np.abs(1 - s) >= G.GRAD_BAND).all() and (s > 1).any() and (s < 1).any()
        assert GOLD["g64__%s__u" % layout].dtype == np.float64
    assert 0 < float(GOLD["meta_grad_envelope"][0]) < 1e-4 and float(GOLD["meta_restatement"][0]) <= 1e-6
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "packing.npz")) < (1 << 20)
