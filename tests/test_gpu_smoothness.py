"""The smoothness prior on the device (csrc/smoothness.hip, pbr_smoothness_step; pypbr_amd.priors) against the oracle of its definition
(tools/smoothness_oracle.py, float64).

Shapes, sized from N.SMOOTH_BLOCK (4 waves of 63 units + 1 halo unit) and N.SMOOTH_BAND_ROWS: 1x1, 1x5, 5x1, 2x2; 23x35 (no whole quads: the
element path); 24x36 (the quad path) and the same through a view one element into its allocation (the element path); widths of 63 + 2 and
63 x 4 + 3 pixels (element path) and 4 x (63 + 2) and 4 x (63 x 4 + 1) pixels (quad path), which put a wave-strip boundary and a workgroup
boundary inside the row; a height of SMOOTH_BAND_ROWS + 1, which puts a band boundary inside the map -- at every band length, since the
bands of a launch are halved (32, 16, 8, 4 rows) while it has fewer than SMOOTH_MIN_BLOCKS workgroups: the small sets walk bands of 4
rows, a batch of SMOOTH_MIN_BLOCKS / 2 images of two bands each walks bands of the full 32.  Inputs are piecewise constant with
patches where s = 0 exactly and a third of the pixels moved by about eps; weights absent, per image and shared, a third of them exactly 0.

Banded (tests/test_gpu_adam.py's rule): the gradient times B H W / lambda, whose values are O(1), and the relative loss within 4 x the
float32 oracle's own error on the same set, covered by the smallest of 1e-6, 2e-6, 1e-5.  A float16 gradient lies within one float16 ulp
of the oracle's value.  terms.sum() against loss: every term is rounded once (2^-24 relative) and so is the loss: 2^-23 |loss|.

Exact, no tolerance: the loss and the gradients of a constant map are 0; gradients where w and the left and upper neighbours' w are 0
are 0; wrap=True on a map rolled by (3, 5) gives the rolled gradient; guard bands of 256 elements around every gradient block are
untouched, parameters and weights unchanged; two runs give the same bits; an upstream gradient of 0.5 halves every gradient; five
replays of a captured fit step with the prior equal five eager steps bit for bit.

MEASURED (MI355X; every run prints its figures before anything is asserted), the worst of each group, float32 oracle's own error ->
band -> device: gradient / k over 223 float32 sets 2.48e-7 -> 1e-6 -> 2.48e-7 (135 sets), 4.94e-7 -> 2e-6 -> 4.94e-7 (81 sets),
6.66e-7 -> 1e-5 -> 6.66e-7 (7 sets) -- in every set the device's distance is the float32 oracle's to the printed digits; relative loss
over 433 sets 1.13e-7 -> 1e-6 -> 1.11e-7; float16 gradients over 210 sets 0.5 ulp.
The loss of four entries against the sum of the oracle's values 7.3e-9, terms.sum() against loss 1.9e-8; the composition against the
one pass: loss 0, gradient / k 2.7e-7."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import photometric_cases as C  # noqa: E402
import smoothness_oracle as S  # noqa: E402

from pypbr_amd import _native as N  # noqa: E402
from pypbr_amd import capture, priors  # noqa: E402
from pypbr_amd import functional as F  # noqa: E402
from pypbr_amd._upload import pack_maps  # noqa: E402
from pypbr_amd.losses import MultiLightRenderingLoss  # noqa: E402
from pypbr_amd.optim import MaterialAdam, material_param_groups  # noqa: E402
from pypbr_amd.priors import LAUNCHES, MaterialSmoothness, smoothness  # noqa: E402

pytestmark = pytest.mark.gpu

EDGE, G = -777.0, 256
BANDS = (1e-6, 2e-6, 1e-5)
LAM, EPS = 0.7, 1e-3
WAVES, STRIP, ROWS = N.SMOOTH_BLOCK // 64, 63, N.SMOOTH_BAND_ROWS
KIND_WRAP = [("l2", False), ("l2", True), ("charbonnier", False), ("charbonnier", True)]
# (H, W, misalign): what each is for is in the docstring
SIZES = {"1x1": (1, 1, 0), "1x5": (1, 5, 0), "5x1": (5, 1, 0), "2x2": (2, 2, 0), "element": (23, 35, 0), "quad": (24, 36, 0), "quad_view": (24, 36, 1),
         "element_strip": (5, STRIP + 2, 0), "element_group": (ROWS + 1, STRIP * WAVES + 3, 0),
         "quad_strip": (5, 4 * (STRIP + 2), 0), "quad_group": (ROWS + 1, 4 * (STRIP * WAVES + 1), 0), "bands": (2 * ROWS + 3, 36, 0)}
TALL = {"element_tall": (ROWS + 1, STRIP + 2, 0), "quad_tall": (ROWS + 1, 4 * (STRIP + 2), 0)}       # with a batch that fills the launch: bands of ROWS rows


def band_of(err32, what):
    """The smallest of BANDS that covers 4 x the float32 oracle's own error."""
    fits = [b for b in BANDS if b >= 4.0 * err32]
    assert fits, "%s: the float32 oracle itself is %.2e from float64: no band covers it" % (what, err32)
    return fits[0]


def guarded(values, dtype, misalign=0):
    """`values` (numpy) as a device tensor of `dtype` inside EDGE margins of G elements, `misalign` elements off the allocation's alignment."""
    n = values.size
    buf = torch.full((n + 2 * G + misalign,), EDGE, dtype=dtype, device="cuda")
    view = buf[G + misalign:G + misalign + n].view(values.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(dtype))
    return buf, view


def guards_intact(buf, view):
    lo = view.storage_offset()
    return bool((buf[:lo] == EDGE).all()) and bool((buf[lo + view.numel():] == EDGE).all())


def make_map(rng, shape, half):
    """Piecewise constant (cells of 3 x 4 pixels, steps O(1)), a third of the pixels moved by (-2 ... 2) eps, a patch left constant; returned
    as the float64 values the device holds."""
    H, W = shape[-2:]
    cells = rng.uniform(0.1, 0.9, shape[:-2] + (-(-H // 3), -(-W // 4)))
    p = np.repeat(np.repeat(cells, 3, axis=-2), 4, axis=-1)[..., :H, :W].copy()
    move = rng.uniform(size=shape) < 1.0 / 3.0
    p[move] += rng.uniform(-2.0, 2.0, int(move.sum())) * EPS
    if H >= 4 and W >= 5:
        p[..., 1:3, 1:4] = 0.25                                                    # s = 0 exactly on (1, 1), (1, 2)
    return p.astype(np.float16 if half else np.float32).astype(np.float64)


def make_weights(rng, shape, mode):
    if mode == "none":
        return None
    B = shape[0] if len(shape) == 4 else 1
    w = rng.uniform(0.0, 1.0, ((B, 1) if mode == "image" and len(shape) == 4 else (1,)) + tuple(shape[-2:]))
    w[rng.uniform(size=w.shape) < 1.0 / 3.0] = 0.0
    if shape[-2] >= 5 and shape[-1] >= 6:
        w[..., 2:5, 2:6] = 0.0                                                     # (3..4, 3..5): w, left and upper w all 0
    return w.astype(np.float32).astype(np.float64)


def compare(what, got_loss, got_grad, p, lam, kind, wrap, w, reduction, half):
    """The device's value and gradient against the float64 oracle under the banding rule; returns the distances."""
    v64, g64 = S.evaluate(p, lam, kind, EPS, wrap, w, reduction)
    v32, g32 = S.evaluate(p, lam, kind, EPS, wrap, w, reduction, dtype=np.float32)
    k = S.scale(lam, p.shape, reduction)
    rel = (lambda v: abs(v - v64) / v64) if v64 != 0 else (lambda v: abs(v))
    loss_band = band_of(rel(v32), what + " loss")
    d_loss = rel(float(got_loss))
    line = "%s: loss %.3e (float32 oracle %.2e, band %.0e)" % (what, d_loss, rel(v32), loss_band)
    if got_grad is not None:
        g = got_grad.detach().cpu().numpy()
        if half:
            assert g.dtype == np.float16
            ulp = np.spacing(np.abs(g64).astype(np.float16)).astype(np.float64)
            worst = float((np.abs(g.astype(np.float64) - g64) / ulp).max())
            print(line + "; float16 gradient %.3f ulp" % worst)
            assert worst <= 1.0
        else:
            err32 = float(np.abs(g32 - g64).max()) / k
            band = band_of(err32, what + " gradient")
            d = float(np.abs(g.astype(np.float64) - g64).max()) / k
            print(line + "; gradient / k %.3e (float32 oracle %.2e, band %.0e)" % (d, err32, band))
            assert d <= band
    else:
        print(line)
    assert d_loss <= loss_band
    return v64, g64


def run_single(name, half, seed, B=1, C=3):
    """One entry per launch through priors._step, every tensor inside guard bands: both kinds, both boundary rules, the three weight modes."""
    H, W, misalign = SIZES[name] if name in SIZES else TALL[name]
    rng = np.random.default_rng(seed)
    dt = torch.float16 if half else torch.float32
    shape = (C, H, W) if B == 1 else (B, C, H, W)
    for kind, wrap in KIND_WRAP:
        for mode in ("none", "image", "shared"):
            p0, w0 = make_map(rng, shape, half), make_weights(rng, shape, mode)
            bp, p = guarded(p0, dt, misalign)
            bg, g = guarded(np.zeros(shape), dt, misalign)
            g.fill_(EDGE)                                                          # every gradient value is WRITTEN
            bw, w = (None, None) if w0 is None else guarded(w0, torch.float32, misalign)
            p_before, w_before = p.clone(), None if w is None else w.clone()
            k = S.scale(LAM, shape, "mean")
            before = LAUNCHES["smoothness_step"]
            loss, terms = priors._step([p], [g], [w], [k], priors.KINDS[kind], EPS, wrap)
            loss2, terms2 = priors._step([p], [None], [w], [k], priors.KINDS[kind], EPS, wrap)      # value only
            first = g.clone()
            loss3, _ = priors._step([p], [g], [w], [k], priors.KINDS[kind], EPS, wrap)
            torch.cuda.synchronize()
            assert LAUNCHES["smoothness_step"] == before + 3
            assert guards_intact(bp, p) and guards_intact(bg, g) and (bw is None or guards_intact(bw, w))
            assert torch.equal(p, p_before) and (w is None or torch.equal(w, w_before))
            assert torch.equal(loss, loss2) and torch.equal(loss, loss3) and torch.equal(first, g) and torch.equal(terms, terms2)     # the same bits
            assert terms.shape == (1,) and terms[0].item() == loss.item()
            what = "%s %s%s %s wrap=%d w=%s" % (name, "fp16" if half else "fp32", "" if B == 1 else " B=%d" % B, kind, wrap, mode)
            _, g64 = compare(what, loss, g, p0, LAM, kind, wrap, w0, "mean", half)
            if w0 is not None and not wrap:
                wz = np.broadcast_to(w0.reshape((-1, 1, H, W)), (B, 1, H, W))
                dead = (wz == 0) & (np.roll(wz, 1, 3) == 0) & (np.roll(wz, 1, 2) == 0)
                dead[..., 0, :] = False
                dead[..., :, 0] = False
                dead = np.broadcast_to(dead, (B, C, H, W)).reshape(shape)
                assert not g.cpu().numpy()[dead].any() and not g64[dead].any()    # exactly 0, in the definition and on the device


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", list(SIZES))
def test_one_entry_against_the_oracle(name, half):
    run_single(name, half, 100 + list(SIZES).index(name))


@pytest.mark.parametrize("channels", [1, 2, 4])
def test_other_channel_counts(channels):
    run_single("element", False, 150 + channels, C=channels)
    run_single("quad", True, 160 + channels, C=channels)


def test_batch_of_two_with_weights_per_image():
    run_single("quad", False, 170, B=2)
    run_single("element", True, 171, B=2)


@pytest.mark.parametrize("name,half", [("element_tall", False), ("quad_tall", True)])
def test_bands_of_full_length_when_the_launch_is_large(name, half):
    H, W, _ = TALL[name]
    B = N.SMOOTH_MIN_BLOCKS // 2
    t = torch.zeros(B, 1, H, W, dtype=torch.float16 if half else torch.float32, device="cuda")
    table = (N.SmoothTensor * 1)(priors._entry(t, None, None, 1.0, N.SMOOTH_L2, EPS, False))
    assert N.lib().pbr_smoothness_workspace_bytes(table, 1) == 4 * B * 2                 # two bands per image: ROWS and 1 rows
    run_single(name, half, 175 + int(half), B=B, C=1)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_a_constant_map_has_no_loss_and_no_gradient(half):
    dt = torch.float16 if half else torch.float32
    for (H, W, _), (kind, wrap) in zip([SIZES["quad"], SIZES["element"], SIZES["bands"], SIZES["2x2"]], KIND_WRAP):
        p = torch.full((3, H, W), 0.375, dtype=dt, device="cuda", requires_grad=True)
        loss, terms = smoothness([p], [LAM], kind=kind, wrap=wrap, return_terms=True)
        loss.backward()
        assert loss.item() == 0.0 and terms[0].item() == 0.0 and not p.grad.any()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_wrap_on_a_rolled_map_gives_the_rolled_gradient(half):
    rng = np.random.default_rng(180)
    dt = torch.float16 if half else torch.float32
    for name in ("quad", "element", "quad_strip", "bands"):
        H, W, _ = SIZES[name]
        p0, w0 = make_map(rng, (3, H, W), half), make_weights(rng, (3, H, W), "shared")
        p, w = torch.from_numpy(p0).to(dt).cuda(), torch.from_numpy(w0).float().cuda()
        grads = []
        for q, v in ((p, w), (torch.roll(p, (3, 5), (-2, -1)), torch.roll(w, (3, 5), (-2, -1)))):
            q = q.clone().requires_grad_(True)
            smoothness([q], [LAM], wrap=True, weights=v).backward()
            grads.append(q.grad)
        assert torch.equal(torch.roll(grads[1], (-3, -5), (-2, -1)), grads[0]) and grads[0].any()


def test_one_launch_holds_entries_of_different_channels_sizes_and_dtypes():
    rng = np.random.default_rng(190)
    shapes = [(3,) + SIZES["quad"][:2], (3,) + SIZES["element"][:2], (1,) + SIZES["5x1"][:2], (1, ROWS + 1, STRIP + 2)]
    halves = [False, True, False, True]
    lams = [0.7, 0.3, 1.1, 0.5]
    p0 = [make_map(rng, s, h) for s, h in zip(shapes, halves)]
    w0 = [make_weights(rng, shapes[0], "shared"), None, None, make_weights(rng, shapes[3], "shared")]
    ps = [guarded(a, torch.float16 if h else torch.float32) for a, h in zip(p0, halves)]
    gs = [guarded(np.zeros(s), torch.float16 if h else torch.float32) for s, h in zip(shapes, halves)]
    ws = [None if a is None else torch.from_numpy(a).float().cuda() for a in w0]
    before = LAUNCHES["smoothness_step"]
    loss, terms = priors._step([v for _, v in ps], [v for _, v in gs], ws, [S.scale(l, s, "mean") for l, s in zip(lams, shapes)],
                               priors.KINDS["charbonnier"], EPS, False)
    torch.cuda.synchronize()
    assert LAUNCHES["smoothness_step"] == before + 1
    assert all(guards_intact(b, v) for b, v in ps + gs)
    total = 0.0
    for i in range(4):
        v64, _ = compare("entry %d of 4" % i, terms[i], gs[i][1], p0[i], lams[i], "charbonnier", False, w0[i], "mean", halves[i])
        total += v64
    d = abs(terms.double().sum().item() - float(loss)) / float(loss)
    print("loss against the sum of the oracle's values %.2e; terms.sum() against loss %.2e (2^-23 = 1.19e-7)" % (abs(float(loss) - total) / total, d))
    assert abs(float(loss) - total) / total <= 1e-6 and d <= 2.0 ** -23


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_batched_views_of_a_material_major_packing(half):
    """B = 2 through pack_maps(material_major=True): batch strides beyond C H W, the maps of the two materials interleaved in one arena;
    through the public call and autograd."""
    rng = np.random.default_rng(200)
    dt = torch.float16 if half else torch.float32
    for h, w in ((24, 36), (23, 35)):
        shapes = [(2, 3, h, w), (2, 1, h, w)]
        p0 = [make_map(rng, s, half) for s in shapes]
        w0 = make_weights(rng, shapes[0], "image")
        views = pack_maps(*[torch.from_numpy(a).to(dt).cuda() for a in p0], material_major=True)
        assert all(v.stride(0) > v.shape[1] * h * w and not v.is_contiguous() for v in views)
        for v in views:
            v.requires_grad_(True)
        before = LAUNCHES["smoothness_step"]
        loss, terms = smoothness(views, [0.7, 0.4], weights=torch.from_numpy(w0).float().cuda(), return_terms=True)
        loss.backward()
        assert LAUNCHES["smoothness_step"] == before + 1
        for i, lam in enumerate((0.7, 0.4)):
            compare("packed %dx%d map %d" % (h, w, i), terms[i], views[i].grad, p0[i], lam, "charbonnier", False, w0, "mean", half)
            assert torch.equal(views[i].detach().cpu().double(), torch.from_numpy(p0[i]))


def test_nine_entries_take_two_launches_and_dropped_entries_none():
    rng = np.random.default_rng(210)
    shapes = [(1 + i % 3, 5 + i, 7 + 2 * i) for i in range(N.MAX_SMOOTH_TENSORS + 1)]
    p0 = [make_map(rng, s, False) for s in shapes]
    ts = [torch.from_numpy(a).float().cuda().requires_grad_(True) for a in p0]
    lams = [0.1 * (i + 1) for i in range(len(ts))]
    before = LAUNCHES["smoothness_step"]
    loss, terms = smoothness(ts, lams, kind="l2", return_terms=True)
    loss.backward()
    assert LAUNCHES["smoothness_step"] == before + 2 and terms.shape == (len(ts),)
    total = 0.0
    for i in range(len(ts)):
        total += compare("entry %d of 9" % i, terms[i], ts[i].grad, p0[i], lams[i], "l2", False, None, "mean", False)[0]
    assert abs(float(loss) - total) / total <= 1e-6
    lams[2] = lams[5] = 0.0                                                        # dropped: 7 entries, one launch, zeros in their places
    before = LAUNCHES["smoothness_step"]
    with torch.no_grad():
        loss7, terms7 = smoothness(ts, lams, kind="l2", return_terms=True)
    assert LAUNCHES["smoothness_step"] == before + 1 and terms7[2].item() == 0.0 == terms7[5].item()
    keep = [i for i in range(len(ts)) if i not in (2, 5)]
    assert torch.equal(terms7[keep], terms[keep]) and not loss7.requires_grad


@functools.lru_cache(maxsize=None)
def fit_case():
    """tests/test_gpu_adam.py's fit: the rendered case of tools/photometric_cases.py, 24 x 36, L = 8."""
    c = C.lambertian("gentle")
    H, W = C.SIZE
    known = [torch.from_numpy(c.albedo.astype(np.float32)).cuda(), torch.from_numpy(c.normal.astype(np.float32)).cuda(),
             torch.full((1, H, W), C.ROUGHNESS, device="cuda"), torch.zeros(1, H, W, device="cuda")]
    lights = torch.from_numpy(c.light).float()
    targets = F.cook_torrance_stack(*known, albedo_is_srgb=False, view_dir=[0.0, 0.0, 1.0], light=lights, light_intensity=c.intensity.tolist(),
                                    light_type="point", light_size=C.LIGHT_SIZE)
    loss = MultiLightRenderingLoss(light_type="point", view_dir=torch.tensor([0.0, 0.0, 1.0]), lights=lights,
                                   light_intensities=torch.tensor(c.intensity.tolist(), dtype=torch.float32), light_size=C.LIGHT_SIZE)
    kw = dict(light=c.light, light_intensity=c.intensity, light_size=C.LIGHT_SIZE)
    confidence = capture.photometric_stereo(targets, None, **kw)[2]
    return targets, loss, kw, (1.0 - confidence).contiguous()


LAMBDAS = {"albedo": 0.05, "normal": 0.02, "roughness": 0.3, "metallic": 0.3, "height": 1.0}


def test_material_smoothness_equals_smoothness_on_the_maps():
    targets, _, kw, weights = fit_case()
    material = capture.initial_material(targets, None, 0.4, **kw)
    groups = material_param_groups(material, lr=1e-2)
    maps = material.__dict__["_store"]
    names = [k for k in ("albedo", "normal", "roughness", "metallic") if k in maps]
    assert len(names) == 4 and len(groups) == 4
    before = LAUNCHES["smoothness_step"]
    loss = MaterialSmoothness(LAMBDAS)(material, weights=weights)
    assert LAUNCHES["smoothness_step"] == before + 1 and loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    got = {k: maps[k].grad.clone() for k in names}
    for k in names:
        maps[k].grad = None
    same, terms = smoothness([maps[k] for k in names], [LAMBDAS[k] for k in names], weights=weights, return_terms=True)
    same.backward()
    assert torch.equal(same, loss) and all(torch.equal(got[k], maps[k].grad) for k in names)
    for i, k in enumerate(names):
        compare("initial material %s" % k, terms[i], maps[k].grad, maps[k].detach().cpu().double().numpy(), LAMBDAS[k], "charbonnier", False,
                weights.cpu().double().numpy(), "mean", False)
    assert float(terms[0]) > 0 and float(terms[1]) > 0 and float(terms[2]) == 0.0  # the constant roughness plane


def test_an_upstream_gradient_of_one_half_halves_every_gradient_and_no_gradient_means_value_only():
    rng = np.random.default_rng(220)
    p0 = [make_map(rng, (3, 24, 36), False), make_map(rng, (1, 23, 35), True)]
    ts = [torch.from_numpy(p0[0]).float().cuda(), torch.from_numpy(p0[1]).half().cuda()]
    grads = []
    for factor in (1.0, 0.5):
        for t in ts:
            t.requires_grad_(True)
            t.grad = None
        (smoothness(ts, [0.7, 0.4], reduction="sum") * factor).backward()
        grads.append([t.grad.clone() for t in ts])
    assert all(torch.equal(h, f * 0.5) and f.any() for f, h in zip(*grads))
    for t in ts:
        t.requires_grad_(False)
    value = smoothness(ts, [0.7, 0.4], reduction="sum")
    assert not value.requires_grad and value.grad_fn is None
    total = S.evaluate(p0[0], 0.7, reduction="sum")[0] + S.evaluate(p0[1], 0.4, reduction="sum")[0]
    assert abs(float(value) - total) / total <= 1e-6
    # twice through one graph: the second backward evaluates again and gives the same bits
    ts[0].requires_grad_(True)
    ts[0].grad = None
    loss = smoothness(ts[:1], [0.7])
    loss.backward(retain_graph=True)
    once = ts[0].grad.clone()
    ts[0].grad = None
    loss.backward()
    assert torch.equal(ts[0].grad, once)


def test_weights_that_require_grad_take_the_composition_and_agree():
    """ATen's float32 order is not the oracle's: held to the widest band of the rule, 1e-5, on the relative loss and on gradient / k."""
    rng = np.random.default_rng(230)
    shape = (3, 23, 35)
    p0, w0 = make_map(rng, shape, False), make_weights(rng, shape, "shared")
    k = S.scale(LAM, shape, "mean")
    p = torch.from_numpy(p0).float().cuda().requires_grad_(True)
    w = torch.from_numpy(w0).float().cuda().requires_grad_(True)
    before = LAUNCHES["smoothness_step"]
    loss = smoothness([p], [LAM], weights=w)
    loss.backward()
    assert LAUNCHES["smoothness_step"] == before and w.grad is not None and w.grad.shape == w.shape
    slow, slow_grad = loss.detach().clone(), p.grad.clone()
    p.grad = None
    fast = smoothness([p], [LAM], weights=w.detach())
    fast.backward()
    assert LAUNCHES["smoothness_step"] == before + 1
    d_loss, d_grad = abs(float(slow) - float(fast)) / float(fast), float((slow_grad - p.grad).abs().max()) / k
    print("composition against the one pass: loss %.2e, gradient / k %.2e" % (d_loss, d_grad))
    assert d_loss <= 1e-5 and d_grad <= 1e-5
    # the weights' gradient is k phi: against the oracle's value through sum(w dR/dw) = R
    assert abs(float((w.grad * w.detach()).double().sum()) - float(fast)) / float(fast) <= 1e-5
    # a transposed view has no dense rows: the composition again
    q = torch.from_numpy(p0).float().cuda().transpose(-1, -2).requires_grad_(True)
    before = LAUNCHES["smoothness_step"]
    loss_t = smoothness([q], [LAM])
    assert LAUNCHES["smoothness_step"] == before
    want = S.evaluate(np.swapaxes(p0, -1, -2), LAM)[0]
    assert abs(float(loss_t) - want) / want <= 1e-5


def fit_step(material, targets, loss_fn, prior, weights, opt):
    opt.zero_grad(set_to_none=True)
    loss = loss_fn(material, targets) + prior(material, weights=weights)
    loss.backward()
    opt.step()
    return loss


def fitted(replay, steps=5):
    """3 warm-up steps, then `steps` more, eager or as replays of one captured step (one stream, no parallel branches)."""
    targets, loss_fn, kw, weights = fit_case()
    material = capture.initial_material(targets, None, 0.4, **kw)
    groups = material_param_groups(material, lr=5e-3, lr_normal=5e-3)
    opt = MaterialAdam(groups, capturable=True)
    prior = MaterialSmoothness(LAMBDAS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fit_step(material, targets, loss_fn, prior, weights, opt)
    torch.cuda.current_stream().wait_stream(side)
    losses = []
    if replay:
        opt.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = fit_step(material, targets, loss_fn, prior, weights, opt)
        for _ in range(steps):
            graph.replay()
            losses.append(loss.detach().clone())
    else:
        for _ in range(steps):
            losses.append(fit_step(material, targets, loss_fn, prior, weights, opt).detach().clone())
    torch.cuda.synchronize()
    params = [g["params"][0] for g in groups]
    return torch.stack(losses), [p.detach().clone() for p in params], [opt.state[p]["exp_avg"].clone() for p in params]


def test_captured_fit_step_with_the_prior_replays_equal_eager_steps_bit_for_bit():
    eager, graph = fitted(False), fitted(True)
    assert torch.equal(eager[0], graph[0]) and torch.isfinite(eager[0]).all()
    for k in (1, 2):
        assert all(torch.equal(a, b) for a, b in zip(eager[k], graph[k]))
