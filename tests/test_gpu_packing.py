"""Packed material tensors on the device (csrc/packing.hip): MaterialBase.from_tensor / as_tensor / normal_rgb against what the real
reference made (tests/golden/packing.npz, tools/gen_packing_golden.py), the layout of the maps, the access patterns of the kernel, guard
bands through the C ABI, gradients against upstream's float64 autograd, and a rendering-loss step from a packed tensor.

Tolerances: affine planes and 3-channel normals are bit-equal (torch.equal).  2-channel normals: 1e-6 absolute, which the generator proved
attainable for the kernel's operation order on every stored value (meta_restatement, 1.2e-7).  Gradients: 4 x meta_grad_envelope x
max(1, |fp64|), the envelope being upstream's own fp32-against-fp64 error on the same inputs."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_packing_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "packing.npz"))
ENVELOPE = float(GOLD["meta_grad_envelope"][0])
SIZES = [G.size_key(hw) for hw in G.SIZES]


def gold(key):
    return torch.from_numpy(GOLD[key])


def classes():
    from pypbr_amd import materials as M
    return {"metallic": M.BasecolorMetallicMaterial, "specular": M.DiffuseSpecularMaterial}


def aten_unpack(t, names, is_normalized):
    """from_tensor as the tutorial's user writes it by hand: slice, clone, affine, z, normalise (any dtype, any device)."""
    out, c = {}, 0
    for name, k in names:
        m = t[..., c:c + k, :, :].clone()
        if is_normalized:
            m = m * 0.5 + 0.5
        if (name, k) == ("normal", 2):
            v = m * 2 - 1
            z = torch.sqrt(torch.clamp(1.0 - (v ** 2).sum(-3, keepdim=True), min=1e-6))
            m = TF.normalize(torch.cat([v, z], dim=-3), dim=-3)
        out[name] = m
        c += k
    return out


# ---- 1. from_tensor against the golden ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("layout", list(G.LAYOUTS))
@pytest.mark.parametrize("cls", ["metallic", "specular"])
def test_from_tensor_equals_the_reference(cls, layout, size):
    names = G.LAYOUTS[layout][1]
    for mode, isn in (("u", False), ("n", True)):
        packed = gold("in__" + size)
        src = G.take(G.normalized(packed) if isn else packed, layout).cuda()
        keep = src.clone()
        m = classes()[cls].from_tensor(src, names=names, is_normalized=isn)
        assert type(m) is classes()[cls] and m.device == src.device and list(m._raw.keys()) == [n for n, _ in names]
        maps = {k: v for k, v in m._raw.items()}
        src.fill_(7.0)                                                                  # the maps are not views of the input
        for name, k in names:
            want = gold("ft__%s__%s__%s__%s__%s" % (cls, layout, mode, size, name))
            got = maps[name].cpu()
            assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape)
            if (name, k) == ("normal", 2):
                err = (got - want).abs().max().item()
                print("\n[from_tensor %s %s %s %s] normal: max |hip - upstream| = %.3e" % (cls, layout, mode, size, err))
                assert err <= 1e-6, (layout, mode, size, err)
            else:
                assert torch.equal(got, want), (layout, mode, size, name)
        # a CPU tensor: the maps are handed out on `device`, the same values
        home = classes()[cls].from_tensor(keep.cpu(), names=names, is_normalized=isn)
        assert home.device == torch.device("cpu")
        for name, _ in names:
            assert home._maps[name].device.type == "cpu" and torch.equal(home._maps[name], maps[name].cpu()), name


@pytest.mark.parametrize("mode, isn", [("u", False), ("n", True)])
def test_from_tensor_near_the_unit_circle(mode, isn):
    from pypbr_amd.materials import BasecolorMetallicMaterial
    src = gold("nc_in")
    src = (G.normalized(src) if isn else src).cuda()
    got = BasecolorMetallicMaterial.from_tensor(src, names=[("normal", 2)], is_normalized=isn).normal.cpu()
    err = (got - gold("nc_out__" + mode)).abs().max().item()
    print("\n[near circle %s] max |hip - upstream| = %.3e over %d values" % (mode, err, got.numel()))
    assert err <= 1e-6, err
    assert np.abs(G.restate_normal_xy(src.cpu().numpy(), isn) - got.numpy()).max() == 0.0      # the kernel IS the restated order


# ---- 2. as_tensor against the golden --------------------------------------------------------------------------------------------------
def _golden_material(size, device="cuda"):
    """The material the generator packed: the reference's from_tensor maps, filed as they are (a 3-channel normal is stored as given)."""
    from pypbr_amd.materials import BasecolorMetallicMaterial
    names = G.LAYOUTS["full9"][1]
    maps = [gold("ft__metallic__full9__u__%s__%s" % (size, name)) for name, _ in names]
    config = [(name, t.shape[0]) for (name, _), t in zip(names, maps)]
    return BasecolorMetallicMaterial.from_tensor(torch.cat(maps).to(device), names=config)


@pytest.mark.parametrize("size", SIZES)
def test_as_tensor_equals_the_reference(size):
    for device in ("cuda", "cpu"):
        m = _golden_material(size, device)
        for case, (names, normalize) in G.AS_CASES.items():
            got = m.as_tensor(names=names, normalize=normalize)
            assert got.device.type == device
            assert torch.equal(got.cpu(), gold("at__%s__%s" % (size, case))), (size, case, device)
        rgb = m.normal_rgb
        assert rgb.device.type == device and torch.equal(rgb.cpu(), (gold("ft__metallic__full9__u__%s__normal" % size) + 1.0) * 0.5)


def test_as_tensor_sees_what_a_reader_of_the_maps_sees():
    from pypbr_amd.io import load_material_from_folder
    m = _golden_material("37x53").tile(2, lazy=True)
    assert m.lazy_tile == (2, 2)
    for case, (names, normalize) in G.AS_CASES.items():
        pending = _golden_material("37x53").tile(2, lazy=True)
        assert torch.equal(pending.as_tensor(names=names, normalize=normalize).cpu(), gold("at__37x53__" + case).repeat(1, 2, 2)), case
    # a material from image files: the normal map's decode is still deferred when as_tensor is called
    folder = os.path.join(ROOT, "tests", "golden", "tiles")
    a, b = load_material_from_folder(folder, preferred_workflow="metallic"), load_material_from_folder(folder, preferred_workflow="metallic")
    assert a.__dict__.get("_raw_normal"), "the fixture is meant to arrive with its normal map undecoded"
    got = a.as_tensor()
    seen = b._maps
    assert got.device == a.device and torch.equal(got.cpu(), torch.cat([seen[k].cpu() for k in seen]))
    assert torch.equal(a.as_tensor(names=[("normal", 3), "roughness"], normalize=True).cpu(),
                       torch.cat([seen["normal"].cpu(), (seen["roughness"].cpu() - 0.5) / 0.5]))


# ---- 3. layout ------------------------------------------------------------------------------------------------------------------------
def _count_calls(monkeypatch):
    from pypbr_amd import _packing
    calls = []
    real = _packing._plane_ops_call

    def counted(ops, *a, **kw):
        calls.append((len(ops), bool(kw.get("backward", a[4] if len(a) > 4 else False))))
        return real(ops, *a, **kw)
    monkeypatch.setattr(_packing, "_plane_ops_call", counted)
    return calls


def test_maps_share_one_allocation_and_one_launch(monkeypatch):
    from pypbr_amd import materials as M
    calls = _count_calls(monkeypatch)
    names = G.LAYOUTS["full9"][1]
    src = gold("in__37x53").cuda()
    m = M.BasecolorMetallicMaterial.from_tensor(src, names=names)
    assert calls == [(8, False)]                                 # 3 + 1 (the 2-channel normal) + 4 planes: one call
    ts = [m._raw[name] for name, _ in names]
    block = M._as_block(ts)
    assert block.data_ptr() == ts[0].data_ptr() and block.shape == (10, 37, 53)
    assert all(t._base is None for t in ts)
    # more than 32 operations: ceil(40 / 32) calls, still one block and the right values
    del calls[:]
    g = torch.Generator().manual_seed(3)
    wide = torch.rand(40, 5, 7, generator=g).cuda()
    config = [("m%d" % i, 1) for i in range(19)] + [("normal", 2)] + [("n%d" % i, 1) for i in range(19)]
    assert sum(k for _, k in config) == 40
    m = M.MaterialBase.from_tensor(wide, names=config, is_normalized=True)
    assert calls == [(32, False), (7, False)]
    want = aten_unpack(wide, config, True)
    for name, k in config:
        if k == 2:
            assert (m._raw[name] - want[name]).abs().max().item() <= 1e-6
        else:
            assert torch.equal(m._raw[name], want[name]), name
    assert M._as_block([m._raw[name] for name, _ in config]).data_ptr() == m._raw["m0"].data_ptr()
    del calls[:]
    m.as_tensor()
    assert calls == [(32, False), (9, False)]


# ---- 4. access patterns ---------------------------------------------------------------------------------------------------------------
def test_views_strides_fp16_and_batches():
    from pypbr_amd import functional as F
    names = G.LAYOUTS["full9"][1]
    g = torch.Generator().manual_seed(11)
    H, W = 37, 53
    t = torch.rand(9, H, W, generator=g).cuda()
    base = F.unpack_planes(t, names, is_normalized=True)
    # a channel-sliced view of a larger tensor: plane stride != H W for its batch, odd offsets
    big = torch.rand(9, 3, H, W, generator=g).cuda()
    big[:, 1] = t
    assert big[:, 1].stride(0) == 3 * H * W
    for got, want in zip(F.unpack_planes(big[:, 1], names, is_normalized=True), base):
        assert torch.equal(got, want)
    wide = torch.zeros(9, H + 3, W + 5, device="cuda")
    wide[:, 1:1 + H, 2:2 + W] = t
    assert not wide[:, 1:1 + H, 2:2 + W].is_contiguous()
    for got, want in zip(F.unpack_planes(wide[:, 1:1 + H, 2:2 + W], names, is_normalized=True), base):
        assert torch.equal(got, want)
    # fp16 storage: the fp32 result of the same (fp16-valued) input, rounded
    th = t.half()
    for got, want in zip(F.unpack_planes(th, names, is_normalized=True), F.unpack_planes(th.float(), names, is_normalized=True)):
        assert got.dtype == torch.float16 and torch.equal(got, want.half())
    assert torch.equal(F.pack_planes([th[:3], th[5:6]], [2, None], [True, False]),
                       F.pack_planes([th[:3].float(), th[5:6].float()], [2, None], [True, False]).half())
    # a batch equals a loop of calls, bit for bit
    t2 = torch.stack([t, torch.rand(9, H, W, generator=g).cuda()])
    batch = F.unpack_planes(t2, names)
    for b in range(2):
        for got, want in zip(batch, F.unpack_planes(t2[b], names)):
            assert got.shape[0] == 2 and torch.equal(got[b], want)
    packed = F.pack_planes(batch, [None, 2, None, None, None, None], [True, False, True, True, True, True])
    for b in range(2):
        assert torch.equal(packed[b], F.pack_planes([m[b] for m in batch], [None, 2, None, None, None, None], [True, False, True, True, True, True]))
    # packing reads views in place too
    assert torch.equal(F.pack_planes([big[0:3, 1], wide[3:5, 1:1 + H, 2:2 + W]]), torch.cat([t[0:3], t[3:5]]))


# ---- 5. guard bands through the C ABI -------------------------------------------------------------------------------------------------
EDGE, FILL = 777.0, -555.0
PIXELS = (1, 3, 4, 5, 7, 8, 127, 128, 130, 1961)


def _guarded(n, lead, margin_value, dtype=torch.float32):
    """A buffer of lead + n + 67 elements: the interior [lead, lead + n) between margins of `margin_value`."""
    buf = torch.full((lead + n + 67,), margin_value, dtype=dtype, device="cuda")
    return buf, buf[lead:lead + n]


def _margins_hold(buf, lead, n, value):
    return bool((buf[:lead] == value).all()) and bool((buf[lead + n:] == value).all())


def _xy_away_from_the_circle(g, pixels):
    xy = torch.randint(0, 256, (2, pixels), generator=g).float() / 255.0
    s = ((xy.double() * 2 - 1) ** 2).sum(0)
    bad = (1 - s).abs() < G.GRAD_BAND
    xy[0, bad], xy[1, bad] = 140.0 / 255.0, 100.0 / 255.0
    return xy


def _ptr(t):
    return t.data_ptr()


@pytest.mark.parametrize("pixels", PIXELS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_forward_writes_its_planes_and_nothing_else(pixels, dtype):
    from pypbr_amd import _native as N, functional as F
    g = torch.Generator().manual_seed(pixels)
    P, es = pixels, torch.empty(0, dtype=dtype).element_size()
    src_buf, src = _guarded(4 * P, 62, float("nan"), dtype)          # planes: a, x, y, b -- back to back, so odd P puts bases off alignment
    values = torch.cat([torch.rand(P, generator=g), _xy_away_from_the_circle(g, P).reshape(-1), torch.rand(P, generator=g)])
    src.copy_(values.to(dtype))
    dst_buf, dst = _guarded(5 * P, 61, EDGE, dtype)                   # planes: a', nx, ny, nz, b'
    dst.fill_(FILL)
    ops = [N.PlaneOp(N.PLANE_AFFINE, 0, _ptr(src), 0, 0, _ptr(dst), 0, 0, None, 0, 0, 0.5, 0.5),
           N.PlaneOp(N.PLANE_NORMAL_XY, 0, _ptr(src) + P * es, 0, P, _ptr(dst) + P * es, 0, P, None, 0, 0, 1.0, 0.0),
           N.PlaneOp(N.PLANE_AFFINE, 0, _ptr(src) + 3 * P * es, 0, 0, _ptr(dst) + 4 * P * es, 0, 0, None, 0, 0, 2.0, -1.0)]
    F._plane_ops_call(ops, 1, P, dtype, src.device)
    torch.cuda.synchronize()
    assert _margins_hold(dst_buf, 61, 5 * P, EDGE) and not bool((dst == FILL).any())
    s32 = src.float().reshape(4, P)
    assert torch.equal(dst[:P], (s32[0] * 0.5 + 0.5).to(dtype)) and torch.equal(dst[4 * P:], (s32[3] * 2 - 1).to(dtype))
    want = aten_unpack(s32[1:3].reshape(2, 1, P), [("normal", 2)], False)["normal"].reshape(3, P)
    err = (dst[P:4 * P].float().reshape(3, P) - want).abs().max().item()
    assert err <= (1e-6 if dtype == torch.float32 else 1e-6 + 2.0 ** -12), err       # fp16: plus half an ulp (2^-11) of a value in [0.5, 1]
    assert torch.isnan(src_buf[:62]).all() and torch.isnan(src_buf[62 + 4 * P:]).all()


@pytest.mark.parametrize("pixels", PIXELS)
def test_backward_writes_every_gradient_once_and_nothing_else(pixels):
    from pypbr_amd import _native as N, functional as F
    g = torch.Generator().manual_seed(100 + pixels)
    P = pixels
    xy_buf, xy = _guarded(2 * P, 63, float("nan"))
    xy.copy_(_xy_away_from_the_circle(g, P).reshape(-1))
    up_buf, up = _guarded(5 * P, 62, float("nan"))                    # upstream: a', nx, ny, nz, b'
    up.copy_(torch.rand(5 * P, generator=g) * 2 - 1)
    gi_buf, gi = _guarded(7 * P, 61, EDGE)                            # gradients: a, x, y, b, c (no upstream), x2, y2 (no upstream)
    gi.fill_(FILL)
    at = lambda t, k: _ptr(t) + 4 * k * P                             # noqa: E731
    ops = [N.PlaneOp(N.PLANE_AFFINE, 0, at(up, 0), 0, 0, at(gi, 0), 0, 0, None, 0, 0, 0.5, 0.5),
           N.PlaneOp(N.PLANE_NORMAL_XY, 0, at(up, 1), 0, P, at(gi, 1), 0, P, at(xy, 0), 0, P, 0.5, 0.5),
           N.PlaneOp(N.PLANE_AFFINE, 0, at(up, 4), 0, 0, at(gi, 3), 0, 0, None, 0, 0, 2.0, -1.0),
           N.PlaneOp(N.PLANE_AFFINE, 0, None, 0, 0, at(gi, 4), 0, 0, None, 0, 0, 2.0, -1.0),
           N.PlaneOp(N.PLANE_NORMAL_XY, 0, None, 0, 0, at(gi, 5), 0, P, None, 0, 0, 1.0, 0.0)]
    # the forward's input under scale 0.5, bias 0.5 is xy * 2 - 1 (is_normalized)
    packed = (xy * 2 - 1).clone()
    xy.copy_(packed)
    F._plane_ops_call(ops, 1, P, torch.float32, xy.device, backward=True)
    torch.cuda.synchronize()
    assert _margins_hold(gi_buf, 61, 7 * P, EDGE) and not bool((gi == FILL).any())
    u = up.reshape(5, P)
    assert torch.equal(gi[:P], u[0] * 0.5) and torch.equal(gi[3 * P:4 * P], u[4] * 2.0)
    assert bool((gi[4 * P:] == 0).all())
    t64 = packed.double().reshape(2, 1, P).requires_grad_()
    (aten_unpack(t64, [("normal", 2)], True)["normal"] * u[1:4].double().reshape(3, 1, P)).sum().backward()
    want = t64.grad.reshape(2, P)
    err = ((gi[P:3 * P].reshape(2, P).double() - want).abs() / want.abs().clamp_min(1.0)).max().item()
    assert err <= 4 * ENVELOPE, (err, ENVELOPE)
    for buf, lead, n in ((xy_buf, 63, 2 * P), (up_buf, 62, 5 * P)):
        assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + n:]).all()


# ---- 6. gradients ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", G.GRAD_LAYOUTS)
@pytest.mark.parametrize("mode, isn", [("u", False), ("n", True)])
def test_from_tensor_gradient_against_upstreams_float64(layout, mode, isn, monkeypatch):
    from pypbr_amd.materials import BasecolorMetallicMaterial
    names = G.LAYOUTS[layout][1]
    base = gold("g_in__" + layout)
    t = (G.normalized(base) if isn else base).cuda().requires_grad_()
    calls = _count_calls(monkeypatch)
    m = BasecolorMetallicMaterial.from_tensor(t, names=names, is_normalized=isn)
    sum((gold("g_w__%s__%s" % (layout, name)).cuda() * m._raw[name]).sum() for name, _ in names).backward()
    assert [c[1] for c in calls] == [False, True]                                     # one launch each way
    g64 = gold("g64__%s__%s" % (layout, mode))
    got = t.grad.cpu().double()
    rel = ((got - g64).abs() / g64.abs().clamp_min(1.0)).max().item()
    ref = ((gold("g32__%s__%s" % (layout, mode)).double() - g64).abs() / g64.abs().clamp_min(1.0)).max().item()
    print("\n[gradient %s %s] hip %.3e, upstream fp32 %.3e, envelope %.3e (bound 4 x)" % (layout, mode, rel, ref, ENVELOPE))
    assert rel <= 4 * ENVELOPE, (rel, ENVELOPE)
    # clamped pairs (1 - s < 1e-6): nothing passes through z -- the gradient is the normalise-only one, with z a constant
    c = sum(k for _, k in names[:[n for n, _ in names].index("normal")])
    x = (t.detach().cpu().double()[c:c + 2] * 0.5 + 0.5) if isn else t.detach().cpu().double()[c:c + 2]
    v = (x * 2 - 1).requires_grad_()
    clamped = (1 - (v.detach() ** 2).sum(0)) < 1e-6
    assert clamped.any() and not clamped.all()
    n = TF.normalize(torch.cat([v, torch.full_like(v[:1], 1e-6).sqrt()]), dim=0)
    (n * gold("g_w__%s__normal" % layout).double()).sum().backward()
    only = v.grad * (1.0 if isn else 2.0)                                             # d v / d t = 2 (x 0.5 under is_normalized)
    err = ((got[c:c + 2] - only).abs() / only.abs().clamp_min(1.0))[:, clamped].max().item()
    assert err <= 4 * ENVELOPE, err
    # a map the loss never touched: its channels receive exactly 0
    t2 = t.detach().clone().requires_grad_()
    m = BasecolorMetallicMaterial.from_tensor(t2, names=names, is_normalized=isn)
    (m._raw["normal"] * gold("g_w__%s__normal" % layout).cuda()).sum().backward()
    untouched = torch.ones(t2.shape[0], dtype=torch.bool)
    untouched[c:c + 2] = False
    assert bool((t2.grad[untouched.cuda()] == 0).all()) and torch.equal(t2.grad[c:c + 2], t.grad[c:c + 2])


def test_as_tensor_gradient_is_exact():
    from pypbr_amd.materials import BasecolorMetallicMaterial
    g = torch.Generator().manual_seed(17)
    H, W = 19, 29
    leaves = {"albedo": torch.rand(3, H, W, generator=g), "roughness": torch.rand(1, H, W, generator=g), "metallic": torch.rand(1, H, W, generator=g)}
    leaves = {k: v.cuda().requires_grad_() for k, v in leaves.items()}
    normal = TF.normalize(torch.rand(3, H, W, generator=g) * 2 - 1, dim=0).cuda().requires_grad_()
    m = BasecolorMetallicMaterial(device=torch.device("cuda"), **leaves)
    m._raw["normal"] = normal
    w = (torch.rand(6, H, W, generator=g) * 2 - 1).cuda()
    (m.as_tensor(names=[("albedo", 2), ("normal", 2), "roughness", "metallic"], normalize=True) * w).sum().backward()
    assert torch.equal(leaves["albedo"].grad[:2], 2 * w[:2]) and bool((leaves["albedo"].grad[2] == 0).all())
    assert torch.equal(normal.grad[:2], w[2:4]) and bool((normal.grad[2] == 0).all())             # normalize skips the normal map
    assert torch.equal(leaves["roughness"].grad, 2 * w[4:5]) and torch.equal(leaves["metallic"].grad, 2 * w[5:6])
    for v in list(leaves.values()) + [normal]:
        v.grad = None
    (m.as_tensor(names=["roughness", ("albedo", 1)]) * w[:2]).sum().backward()
    assert torch.equal(leaves["roughness"].grad, w[0:1]) and torch.equal(leaves["albedo"].grad[0], w[1]) and bool((leaves["albedo"].grad[1:] == 0).all())
    assert leaves["metallic"].grad is None and normal.grad is None


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------
def test_rendering_loss_step_from_a_packed_tensor():
    """A packed tensor that requires grad -> from_tensor(is_normalized=True) -> RenderingLoss -> backward, against the same step built
    from torch slicing and the ATen decode feeding functional.rendering_loss_mse; the tolerances are test_gpu_loss_step.py's for its
    unfused comparison (loss 2e-6 x (1 + loss), gradients 2e-5 x the largest gradient + 1e-9)."""
    from pypbr_amd import functional as F
    from pypbr_amd.losses import RenderingLoss
    from pypbr_amd.materials import BasecolorMetallicMaterial
    g = torch.Generator().manual_seed(23)
    H, W = 37, 53
    names = [("albedo", 3), ("normal", 2), ("roughness", 1), ("metallic", 1)]
    x = torch.randint(0, 256, (7, H, W), generator=g).float() / 255.0
    x[3:5] = _xy_away_from_the_circle(g, H * W).reshape(2, H, W)
    x[5] = 0.15 + 0.85 * x[5]
    target = torch.rand(3, H, W, generator=g).cuda()
    packed = (x * 2 - 1).cuda()

    t = packed.clone().requires_grad_()
    m = BasecolorMetallicMaterial.from_tensor(t, names=names, is_normalized=True)
    loss = RenderingLoss(light_type="point")(m, target)
    loss.backward()

    r = packed.clone().requires_grad_()
    maps = aten_unpack(r, names, True)
    ref = F.rendering_loss_mse(maps["albedo"], maps["normal"], maps["roughness"], maps["metallic"], target=target, view_dir=[0.0, 0.0, 1.0],
                               light=[0.1, 0.1, 1.0], light_intensity=[1.0, 1.0, 1.0], light_type="point")
    ref.backward()
    print("\n[packed loss step] loss %.6f against %.6f, max |grad difference| %.3e of %.3e"
          % (loss.item(), ref.item(), (t.grad - r.grad).abs().max().item(), r.grad.abs().max().item()))
    assert abs(loss.item() - ref.item()) <= 2e-6 * (1 + ref.item())
    assert (t.grad - r.grad).abs().max().item() <= 2e-5 * (float(r.grad.abs().max()) + 1e-12) + 1e-9
