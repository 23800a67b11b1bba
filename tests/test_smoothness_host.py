"""The smoothness prior without a device: the definition (tools/smoothness_oracle.py, float64) against float64 autograd of the plain ATen
composition written out here; pypbr_amd.priors._composition (the ATen form the package itself falls back to) against the oracle; the
float32 oracle against the float64 one; the table entry's layout; every validation code of pbr_smoothness_check / pbr_smoothness_step
(calls that launch nothing); every ValueError of the Python surface; the header's declarations against the binding's export table."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import smoothness_oracle as S  # noqa: E402

import abi_header  # noqa: E402
from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import priors  # noqa: E402
from pypbr_amd.materials import BasecolorMetallicMaterial  # noqa: E402

SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (23, 35)]
LAM, EPS = 0.7, 1e-3


def aten_reference(p, lam, kind, eps, wrap, w, reduction):
    """The prior as a user would write it: two shifted differences, squares, a channel sum, a square root, a weighted mean."""
    x = p if p.dim() == 4 else p[None]
    B, C, H, W = x.shape
    if wrap:
        dx, dy = torch.roll(x, -1, 3) - x, torch.roll(x, -1, 2) - x
    else:
        dx, dy = torch.zeros_like(x), torch.zeros_like(x)
        dx[..., :-1] = x[..., 1:] - x[..., :-1]
        dy[..., :-1, :] = x[..., 1:, :] - x[..., :-1, :]
    s = (dx ** 2 + dy ** 2).sum(1, keepdim=True)
    phi = s if kind == "l2" else torch.sqrt(s + eps ** 2) - eps
    if w is not None:
        phi = phi * w.reshape(-1, 1, H, W)
    return lam * (phi.mean() if reduction == "mean" else phi.sum())


def make_case(rng, B, C, H, W, weights):
    """Values O(1) with a constant patch (s = 0 exactly) and steps around eps; weights with a third exactly 0."""
    shape = (C, H, W) if B == 1 else (B, C, H, W)
    p = rng.uniform(0.0, 1.0, shape)
    small = rng.uniform(size=shape) < 0.3
    p[small] = 0.5 + rng.uniform(-2.0, 2.0, int(small.sum())) * EPS
    if H >= 4 and W >= 4:
        p[..., 1:3, 1:4] = 0.25
    w = None
    if weights != "none":
        w = rng.uniform(0.0, 1.0, (1, H, W) if (weights == "shared" or B == 1) else (B, 1, H, W))
        w[rng.uniform(size=w.shape) < 1.0 / 3.0] = 0.0
    return p, w


CASES = list(itertools.product(SIZES, (1, 3), (1, 2), ("l2", "charbonnier"), (False, True), ("none", "image", "shared")))


def test_oracle_equals_float64_autograd_of_the_aten_composition():
    rng = np.random.default_rng(21)
    worst_loss = worst_grad = 0.0
    for (H, W), C, B, kind, wrap, weights in CASES:
        p, w = make_case(rng, B, C, H, W, weights)
        for reduction in ("mean", "sum"):
            t = torch.tensor(p, dtype=torch.float64, requires_grad=True)
            ref = aten_reference(t, LAM, kind, EPS, wrap, None if w is None else torch.tensor(w), reduction)
            ref.backward()
            value, g = S.evaluate(p, LAM, kind, EPS, wrap, w, reduction)
            k = S.scale(LAM, p.shape, reduction)
            worst_loss = max(worst_loss, abs(value - ref.item()) / max(abs(ref.item()), 1e-300) if ref.item() != 0 else abs(value))
            worst_grad = max(worst_grad, float(np.abs(g - t.grad.numpy()).max()) / k)
    print("float64 oracle against float64 autograd over %d cases: loss (relative) %.2e, gradient / k %.2e" % (2 * len(CASES), worst_loss, worst_grad))
    assert worst_loss <= 1e-12 and worst_grad <= 1e-9


def test_private_composition_equals_the_oracle():
    rng = np.random.default_rng(22)
    worst_loss = worst_grad = 0.0
    for (H, W), C, B, kind, wrap, weights in CASES:
        p, w = make_case(rng, B, C, H, W, weights)
        t = torch.tensor(p, dtype=torch.float64, requires_grad=True)
        tw = None if w is None else torch.tensor(w, requires_grad=True)
        loss, terms = priors._composition([t], [LAM], kind, EPS, wrap, [tw], "mean")
        loss.backward()
        value, g = S.evaluate(p, LAM, kind, EPS, wrap, w, "mean")
        assert terms.shape == (1,) and terms[0].item() == loss.item()
        worst_loss = max(worst_loss, abs(value - loss.item()) / abs(value) if value != 0 else abs(loss.item()))
        worst_grad = max(worst_grad, float(np.abs(g - t.grad.numpy()).max()) / S.scale(LAM, p.shape, "mean"))
        assert tw is None or tw.grad is not None                                   # the weights are differentiable here
    print("priors._composition against the oracle: loss (relative) %.2e, gradient / k %.2e" % (worst_loss, worst_grad))
    assert worst_loss <= 1e-12 and worst_grad <= 1e-9


def test_composition_sums_entries_and_takes_one_weight_for_every_entry_of_its_size():
    rng = np.random.default_rng(23)
    a, b, c = rng.uniform(size=(3, 6, 7)), rng.uniform(size=(1, 6, 7)), rng.uniform(size=(1, 4, 4))
    w = rng.uniform(size=(1, 6, 7))
    loss, terms = priors._composition([torch.tensor(a), torch.tensor(b), torch.tensor(c)], [0.3, 0.2, 0.1], "charbonnier", EPS, False, torch.tensor(w), "sum")
    want = [S.evaluate(a, 0.3, weights=w, reduction="sum")[0], S.evaluate(b, 0.2, weights=w, reduction="sum")[0], S.evaluate(c, 0.1, reduction="sum")[0]]
    assert np.allclose(terms.numpy(), want, rtol=1e-12, atol=0) and abs(loss.item() - sum(want)) <= 1e-12 * sum(want)


def test_float32_oracle_is_close_to_the_float64_oracle_and_exact_where_the_definition_is():
    rng = np.random.default_rng(24)
    p, w = make_case(rng, 2, 3, 23, 35, "image")
    p = p.astype(np.float32).astype(np.float64)
    for kind, wrap in itertools.product(("l2", "charbonnier"), (False, True)):
        v64, g64 = S.evaluate(p, LAM, kind, EPS, wrap, w)
        v32, g32 = S.evaluate(p, LAM, kind, EPS, wrap, w, dtype=np.float32)
        k = S.scale(LAM, p.shape, "mean")
        assert g32.dtype == np.float32 and abs(v32 - v64) <= 1e-6 * v64 and np.abs(g32 - g64).max() / k <= 1e-5
    flat = np.full((3, 7, 9), 0.375)
    for kind, wrap in itertools.product(("l2", "charbonnier"), (False, True)):
        for dtype in (np.float64, np.float32):
            v, g = S.evaluate(flat, LAM, kind, EPS, wrap, dtype=dtype)
            assert v == 0.0 and not g.any()                                        # a constant map: exactly 0, both ways
    # the naive Charbonnier form cancels in float32; the oracle's does not
    s, e = np.float32(1e-10), np.float32(1e-3)
    assert abs(float(s / (np.sqrt(s + e * e) + e)) - 4.99988e-8) < 1e-12 < abs(float(np.sqrt(s + e * e) - e) - 4.99988e-8)


def test_table_entry_layout_and_exported_constants():
    lib = N.lib()
    assert lib.pbr_smooth_tensor_size() == ctypes.sizeof(N.SmoothTensor) == 104
    header = abi_header.RAW
    for name, value in (("PBR_MAX_SMOOTH_TENSORS", N.MAX_SMOOTH_TENSORS), ("PBR_SMOOTH_BLOCK", N.SMOOTH_BLOCK), ("PBR_SMOOTH_BAND_ROWS", N.SMOOTH_BAND_ROWS),
                        ("PBR_SMOOTH_MIN_BAND_ROWS", N.SMOOTH_MIN_BAND_ROWS), ("PBR_SMOOTH_MIN_BLOCKS", N.SMOOTH_MIN_BLOCKS)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
    assert re.search(r"PBR_SMOOTH_L2 = (\d+), PBR_SMOOTH_CHARBONNIER = (\d+)", header).groups() == (str(N.SMOOTH_L2), str(N.SMOOTH_CHARBONNIER))
    assert N.SMOOTH_BLOCK % 64 == 0


BASE = 1 << 20        # addresses that are never touched: none of these calls launches


def entry(**kw):
    f = dict(param=BASE, grad=BASE + (1 << 16), weights=None, param_batch_stride=0, param_plane_stride=64, grad_batch_stride=0, grad_plane_stride=64,
             weights_batch_stride=0, k=1.0, eps=1e-3, dtype=N.F32, batch=1, channels=3, height=8, width=8, kind=N.SMOOTH_CHARBONNIER, wrap=0)
    f.update(kw)
    return N.SmoothTensor(**f)


def check(*entries):
    table = (N.SmoothTensor * max(len(entries), 1))(*entries)
    lib = N.lib()
    rc = lib.pbr_smoothness_check(table, len(entries))
    assert (lib.pbr_smoothness_workspace_bytes(table, len(entries)) == 0) == (rc != N.OK)
    if rc != N.OK:       # the step refuses the same table with the same code, before it looks at anything else
        assert lib.pbr_smoothness_step(table, len(entries), BASE, None, BASE, 1 << 30, None) == rc
    return rc


def test_validation_codes():
    lib = N.lib()
    assert check(entry()) == N.OK
    assert check(entry(grad=None)) == N.OK and check(entry(weights=BASE + (1 << 18))) == N.OK
    assert check(entry(kind=N.SMOOTH_L2, eps=0.0)) == N.OK                         # eps belongs to Charbonnier
    assert lib.pbr_smoothness_check(None, 1) == N.ERR_NULL_MAP
    assert check() == N.ERR_SHAPE and check(*[entry(grad=None)] * (N.MAX_SMOOTH_TENSORS + 1)) == N.ERR_SHAPE
    assert check(entry(param=None)) == N.ERR_NULL_MAP
    assert check(entry(channels=0)) == N.ERR_CHANNELS and check(entry(channels=5)) == N.ERR_CHANNELS
    assert check(entry(dtype=7)) == N.ERR_DTYPE and check(entry(kind=2)) == N.ERR_UNSUPPORTED
    for bad in (dict(batch=0), dict(height=0), dict(width=0), dict(height=(1 << 30) + 1, width=1), dict(width=(1 << 30) + 1, height=1),
                dict(height=1 << 21, width=1 << 20, grad=None, param_plane_stride=1 << 41),
                dict(eps=0.0), dict(eps=-1e-3), dict(eps=float("nan")), dict(k=float("inf")),
                dict(param_batch_stride=-1), dict(param_plane_stride=-1), dict(grad_batch_stride=-1), dict(grad_plane_stride=-1), dict(weights_batch_stride=-1),
                dict(param=BASE + 2), dict(grad=BASE + (1 << 16) + 1), dict(weights=BASE + (1 << 18) + 2), dict(dtype=N.F16, param=BASE + 1)):
        assert check(entry(**bad)) == N.ERR_SHAPE, bad
    assert check(entry(dtype=N.F16, param=BASE + 2, grad=BASE + (1 << 16) + 2)) == N.OK            # float16: 2-byte alignment
    # a gradient may overlap nothing; parameters and weights may overlap each other
    assert check(entry(grad=BASE)) == N.ERR_SHAPE                                   # its own parameter
    assert check(entry(grad=BASE + 4 * 191)) == N.ERR_SHAPE                         # the parameter's last element
    assert check(entry(grad=BASE + 4 * 192)) == N.OK
    assert check(entry(weights=BASE + (1 << 16) + 4 * 64)) == N.ERR_SHAPE           # the weights inside the gradient's second plane
    assert check(entry(grad_plane_stride=63)) == N.ERR_SHAPE                        # the gradient's planes on top of each other
    assert check(entry(), entry()) == N.ERR_SHAPE                                   # two entries, one gradient
    assert check(entry(), entry(grad=BASE + (1 << 17))) == N.OK                     # ... one parameter twice is fine
    assert check(entry(), entry(param=BASE + (1 << 16), grad=BASE + (1 << 17))) == N.ERR_SHAPE      # entry 0's gradient is entry 1's parameter
    # plane by plane: a gradient interleaved with a parameter of wider plane stride (a material-major packing) is accepted
    assert check(entry(param_plane_stride=128, grad=BASE + 4 * 64, grad_plane_stride=128)) == N.OK
    assert check(entry(param_plane_stride=128, grad=BASE + 4 * 63, grad_plane_stride=128)) == N.ERR_SHAPE
    # the step's own pointers
    table = (N.SmoothTensor * 1)(entry())
    need = lib.pbr_smoothness_workspace_bytes(table, 1)
    assert need == 4 * workgroups([(1, 8, 8, True)]) == 8                          # 8 rows in bands of 4: two workgroups, one float32 partial each
    assert lib.pbr_smoothness_step(table, 1, None, None, BASE, need, None) == N.ERR_NULL_MAP
    assert lib.pbr_smoothness_step(table, 1, BASE, None, None, need, None) == N.ERR_NULL_MAP
    assert lib.pbr_smoothness_step(table, 1, BASE, None, BASE, need - 1, None) == N.ERR_SHAPE
    assert lib.pbr_smoothness_step(None, 1, BASE, None, BASE, need, None) == N.ERR_NULL_MAP


def workgroups(entries):
    """The launch's workgroups by the header's rule: images x bands x strip groups per entry -- a strip group is SMOOTH_BLOCK / 64 waves of
    63 units (quads where the entry is whole quads), a band SMOOTH_BAND_ROWS rows, halved down to SMOOTH_MIN_BAND_ROWS while the launch
    has fewer than SMOOTH_MIN_BLOCKS workgroups.  entries: (B, H, W, quads)."""
    waves, rows = N.SMOOTH_BLOCK // 64, N.SMOOTH_BAND_ROWS
    while True:
        total = sum(B * -(-H // rows) * -(-(-(-(W // 4 if quads else W) // 63)) // waves) for B, H, W, quads in entries)
        if total >= N.SMOOTH_MIN_BLOCKS or rows <= N.SMOOTH_MIN_BAND_ROWS:
            return total
        rows //= 2


def test_workspace_counts_the_workgroups():
    lib = N.lib()
    waves, rows = N.SMOOTH_BLOCK // 64, N.SMOOTH_BAND_ROWS

    def one(B, H, W, quads):
        return entry(batch=B, height=H, width=W, grad=None, param_batch_stride=3 * H * W, param_plane_stride=H * W, param=BASE if quads else BASE + 4)
    cases = [[(1, 1, 1, False)], [(2, rows + 1, 63 * waves, False)], [(1, rows, 63 * waves + 1, False)], [(3, 2 * rows, 4 * 63 * waves, True)],
             [(1, 5, 4 * 63 * waves + 4, True)], [(1, 4096, 4096, True)], [(1, 1024, 1024, True)], [(1, 256, 256, True), (2, 100, 35, False)],
             [(1, 1024, 1024, True)] * 2]
    for entries in cases:
        table = (N.SmoothTensor * len(entries))(*[one(*e) for e in entries])
        assert lib.pbr_smoothness_workspace_bytes(table, len(entries)) == 4 * workgroups(entries), entries
    assert workgroups([(1, 4096, 4096, True)]) == 128 * 5 and workgroups([(1, 1024, 1024, True)]) == 64 * 2 * 4      # bands of 32 rows; of 4 rows


def test_value_errors_of_the_python_surface():
    t3, t1 = torch.zeros(3, 4, 6), torch.zeros(1, 4, 6)
    ok = dict(kind="charbonnier", eps=1e-3, wrap=False, weights=None, reduction="mean")
    for args, kw in ((([t3, t1], [0.1]), {}),                                      # lengths
                     (([t3], [0.1, 0.2]), {}),
                     (([t3], [0.1]), dict(kind="tv")),
                     (([t3], [0.1]), dict(reduction="max")),
                     (([t3], [0.1]), dict(eps=0.0)),
                     (([t3], [0.1]), dict(eps=-1.0)),
                     (([t3], [-0.1]), {}),
                     (([t3, t1], [0.1, 0.1]), dict(weights=[None])),               # a sequence of another length
                     (([t3], [0.1]), dict(weights=[torch.zeros(1, 4, 5)])),        # a weight of another size
                     (([t3], [0.1]), dict(weights=[torch.zeros(3, 4, 6)])),        # ... with channels
                     (([t3], [0.1]), dict(weights=[torch.zeros(2, 1, 4, 6)])),     # ... with a batch the map does not have
                     (([t3], [0.1]), dict(weights=torch.zeros(1, 5, 5))),          # one plane that fits no entry
                     (([torch.zeros(5, 4, 6)], [0.1]), {}),                        # channels outside 1..4
                     (([torch.zeros(4, 6)], [0.1]), {})):
        with pytest.raises(ValueError):
            priors.smoothness(*args, **dict(ok, **kw))
        with pytest.raises(ValueError):
            priors._composition(*args, **dict(ok, **kw))
    with pytest.raises(RuntimeError):
        priors.smoothness([t3], [0.1])                                             # CPU tensors: no CPU path
    for kw in (dict(lambdas={"albedo": 0.1, "gloss": 0.1}), dict(lambdas={"albedo": -1.0}), dict(lambdas={"albedo": 0.1}, kind="tv"),
               dict(lambdas={"albedo": 0.1}, eps=0.0), dict(lambdas={"albedo": 0.1}, reduction="max")):
        with pytest.raises(ValueError):
            priors.MaterialSmoothness(**kw)


def test_material_smoothness_refuses_maps_that_are_not_materialised():
    g = torch.Generator().manual_seed(3)
    mat = BasecolorMetallicMaterial(albedo=torch.rand(3, 8, 8, generator=g), roughness=torch.rand(1, 8, 8, generator=g), metallic=torch.rand(1, 8, 8, generator=g))
    prior = priors.MaterialSmoothness({"albedo": 0.1, "roughness": 0.2, "height": 0.3})
    with pytest.raises(RuntimeError):
        prior(mat)                                                                 # materialised, but on the host: no CPU path
    mat.__dict__["_lazy_tile"] = (2, 2)
    with pytest.raises(ValueError, match="materialis"):
        prior(mat)
    mat.__dict__["_lazy_tile"] = (1, 1)
    mat.__dict__["_lazy_blend"] = ({}, None)
    with pytest.raises(ValueError, match="materialis"):
        prior(mat)
    mat.__dict__["_lazy_blend"] = None
    with pytest.raises(ValueError):
        priors.MaterialSmoothness({"specular": 0.1})(mat)                          # nothing of it is stored
