"""Guard bands around every buffer a kernel WRITES: gradients, workspaces, strided and fp16 results, the stand-alone map kernels.

The value tests check what a kernel writes inside its output; these check that it writes ONLY there, and writes all of it.  Every launch goes
through the C ABI (ctypes, plan.desc), because autograd cannot place gradients into caller buffers:
  * inputs sit inside NaN margins (0xFF bytes for integer samples): a read outside an input poisons a checked value;
  * outputs sit inside EDGE margins and their interior is pre-filled with UNWRITTEN, so "every value written" is asserted too (outputs that
    accumulate hold known values instead);
  * workspaces are uint8 buffers of EXACTLY the queried byte count inside 0xA5 margins, the interior 0xFF (NaN as fp32 and fp64): a kernel that
    relies on zeroed workspace, or a size query that promises too little, fails;
  * values are held to a float64 reference (torch_oracle / blend_oracle autograd, the C oracle, ATen) at the tolerances of the value tests, and
    forms that are bit-identical by design to a form so held are compared with torch.equal.
Each case pins the form it ran (plan.kernel_name, pbr_resize_form, the folded workspace size, pbr_blend_backward_serves, or the documented
selection rules of the backward kernels), so coverage cannot drift silently when a rule changes."""
import ctypes

import numpy as np
import pytest
import torch

import blend_oracle as BO
import c_oracle as C
import map_op_cases as MC
import torch_oracle as O

pytestmark = pytest.mark.gpu

G = 256                        # guard elements per side: keeps 16-byte alignment; an odd count moves a view off it
EDGE = -777.0                  # margins of outputs (exact in fp16)
UNWRITTEN = -1234.0            # interior of outputs before the launch (exact in fp16)
WS_EDGE, WS_FILL = 0xA5, 0xFF
NAN = float("nan")
WIDTHS = (1, 3, 4, 5, 7, 8, 127, 128, 130, 256)
WORKFLOWS = ("metallic", "specular", "converted")
CHANNELS = (3, 3, 1, 1, 3)     # albedo, normal, roughness, metallic, specular


def P(t):
    return None if t is None else t.data_ptr()


def _lib():
    from pypbr_amd import _native as N
    return N, N.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(t, fill, g=G):
    """(buffer, view): the values of `t` on the device with `g` elements of `fill` on each side."""
    t = t.reshape(-1).cuda()
    buf = torch.full((t.numel() + 2 * g,), fill, dtype=t.dtype, device="cuda")
    buf[g:g + t.numel()] = t
    return buf, buf[g:g + t.numel()]


class Guards:
    """The buffers of one launch, and the checker: margins intact, inputs untouched, every output value written and finite."""

    def __init__(self, g=G):
        self.g, self.ins, self.outs, self.ws = g, [], [], []

    def input(self, t, g=None):
        g = self.g if g is None else g
        fill = NAN if t.dtype.is_floating_point else -1            # integer samples: every byte 0xFF
        buf, view = guarded(t, fill, g)
        self.ins.append((buf, g, view.clone()))
        return view.view(t.shape)

    def output(self, shape, dtype=torch.float32, init=None, g=None):
        g = self.g if g is None else g
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * g,), EDGE, dtype=dtype, device="cuda")
        buf[g:g + n] = UNWRITTEN if init is None else init.reshape(-1).to(dtype).cuda()
        self.outs.append((buf, g, n, init is None))
        return buf[g:g + n].view(shape)

    def workspace(self, nbytes):
        buf = torch.full((int(nbytes) + 512,), WS_EDGE, dtype=torch.uint8, device="cuda")
        buf[256:256 + nbytes] = WS_FILL
        self.ws.append((buf, int(nbytes)))
        return buf[256:]                                             # data_ptr() is valid also for a 0-byte workspace

    def check(self, tag):
        torch.cuda.synchronize()
        for buf, g, keep in self.ins:
            edge = buf[:g], buf[g + keep.numel():]
            if buf.dtype.is_floating_point:
                assert all(bool(torch.isnan(e).all()) for e in edge), ("input margin written", tag)
            else:
                assert all(bool((e == -1).all()) for e in edge), ("input margin written", tag)
            inner = buf[g:g + keep.numel()]
            assert torch.equal(torch.nan_to_num(inner.float(), 7.0), torch.nan_to_num(keep.float(), 7.0)), ("input written", tag)
        for buf, g, n, fresh in self.outs:
            assert bool((buf[:g] == EDGE).all()) and bool((buf[g + n:] == EDGE).all()), ("output margin written", tag)
            inner = buf[g:g + n]
            if fresh:
                assert not bool((inner == UNWRITTEN).any()), ("output value not written", int((inner == UNWRITTEN).sum()), tag)
            assert bool(torch.isfinite(inner.float()).all()), ("non-finite output", tag)
        for buf, n in self.ws:
            assert bool((buf[:256] == WS_EDGE).all()) and bool((buf[256 + n:] == WS_EDGE).all()), ("workspace margin written", n, tag)


def close64(got, want, tag, rel=2e-5, f16=False, scale=None):
    """|got - want| <= rel * (1 + |want|) against float64 (the backward tests' band); fp16 results add their rounding.  `scale`: the band is
    relative to the largest |want| instead (sums over pixels, loss gradients)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (tag, tuple(got.shape), tuple(want.shape))
    ref = want.abs() + (1.0 if scale is None else float(want.abs().max()) + 1e-30)
    band = rel * ref + (2e-3 * want.abs() + 1e-7 if f16 else 0.0)
    err = (got - want).abs()
    assert bool((err <= band).all()), (tag, float(err.max()), float(want.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# materials and float64 references


def _material(g, B, H, W, workflow, dtype=torch.float32, normal=True):
    a = torch.rand(B, 3, H, W, generator=g)
    n = torch.cat([torch.rand(B, 2, H, W, generator=g) - 0.5, torch.ones(B, 1, H, W)], 1) if normal else None
    r = torch.rand(B, 1, H, W, generator=g) * 0.7 + 0.3
    m = torch.rand(B, 1, H, W, generator=g) if workflow != "specular" else None
    s = torch.rand(B, 3, H, W, generator=g) if workflow == "specular" else None
    return [None if t is None else t.to(dtype) for t in (a, n, r, m, s)]


def _params(light_type, lights, srgb=True, workflow="metallic"):
    L = [[0.1, 0.1, 1.0], [-0.4, 0.2, 0.7], [0.3, -0.3, 0.9]] if light_type == "point" else [[0.3, -0.2, 1.0], [0.1, 0.4, 0.8], [-0.2, 0.1, 1.0]]
    I = [[1.0, 0.9, 0.8], [0.4, 0.5, 0.6], [0.3, 0.35, 0.3]]
    return dict(view_dir=[0.05, 0.1, 0.9], light=L[:lights], light_intensity=I[:lights], light_type=light_type,
                light_size=1.5 if light_type == "point" else None, albedo_is_srgb=srgb, specular_is_srgb=srgb, return_srgb=srgb,
                convert_to_diffuse_specular=(workflow == "converted"))


def _render64(maps, workflow, kw, y_offset=0, H_total=None, view=None, lights=None, intens=None):
    """The reference's forward in float64 per material: [B,C,H,W] maps (None = absent), the light sum of cook_torrance_multi
    (per-light clamp, sum, clamp, encode), the converted workflow through metallic_to_diffuse_specular.  view / lights / intens:
    float64 tensors to differentiate (else the descriptor's values)."""
    a, n, r, m, s = maps
    view = torch.tensor(kw["view_dir"], dtype=torch.float64) if view is None else view
    lights = torch.tensor(kw["light"], dtype=torch.float64).reshape(-1, 3) if lights is None else lights
    intens = torch.tensor(kw["light_intensity"], dtype=torch.float64).reshape(-1, 3) if intens is None else intens
    outs = []
    for b in range(a.shape[0]):
        ab, nb, rb = a[b], None if n is None else n[b], r[b]
        mb, sb = None if m is None else m[b], None if s is None else s[b]
        a_srgb, s_srgb = kw["albedo_is_srgb"], kw["specular_is_srgb"]
        if workflow == "converted":
            ab, sb = O.metallic_to_diffuse_specular(O.srgb_to_linear(ab) if a_srgb else ab, mb)
            mb, a_srgb = None, False
        acc = None
        for i in range(lights.shape[0]):
            c = O.cook_torrance(ab, nb, rb, mb, sb, view=view, light=lights[i], intensity=intens[i if intens.shape[0] > 1 else 0],
                                light_type=kw["light_type"], light_size=kw["light_size"], albedo_is_srgb=a_srgb, specular_is_srgb=s_srgb,
                                return_srgb=False, y_offset=y_offset, H_total=H_total)
            acc = c if acc is None else acc + c
        acc = torch.clamp(acc, 0.0, 1.0)
        outs.append(O.linear_to_srgb(acc) if kw["return_srgb"] else acc)
    return torch.stack(outs)


def _leaves64(maps):
    return [None if t is None else t.double().requires_grad_(True) for t in maps]


def _plan(maps, kw, **extra):
    from pypbr_amd import functional as F
    return F.plan_cook_torrance(*maps, **kw, **extra)


def _launch_backward(plan, gout, grads):
    N, lib = _lib()
    N.check(lib.pbr_cook_torrance_backward(ctypes.byref(plan.desc), P(gout), *[P(t) for t in grads], _stream()))


def backward_form(desc, aligned_4byte=True, with_params=False):
    """The documented selection rules of pbr_cook_torrance_backward (include/pbr_hip.h, ct_backward.hip): "stream" = the streamed kernel (fp16
    maps, one light, untiled, width % 128 == 0, bwd_run != 0, 4-byte aligned planes and gradients; never with the light / view gradients),
    "one-pixel" = the one-pixel body (width < 4, max_vec = 1, the light / view gradients with an odd width), else "vector"."""
    N, _ = _lib()
    t = desc.tuning.contents.knob if desc.tuning else None
    knob = lambda k: None if t is None or t[k] == N.TUNE_UNSET else t[k]
    if (not with_params and desc.map_dtype == N.F16 and desc.n_lights == 1 and not desc.map_height and desc.width % 128 == 0
            and knob(N.TUNE_BWD_RUN) != 0 and aligned_4byte):
        return "stream"
    if desc.width < 4 or knob(N.TUNE_MAX_VEC) == 1 or (with_params and desc.width % 2):
        return "one-pixel"
    return "vector"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. pbr_cook_torrance_backward: every workflow, light type, light count, normal map or none, sRGB on and off; all gradients, each alone


BWD_CASES = [(dt, wf, lt, L, nm, srgb) for dt in ("f32", "f16") for wf in WORKFLOWS for lt in ("point", "directional") for L in (1, 3)
             for nm in (True, False) for srgb in (True, False)]


@pytest.mark.parametrize("dt,workflow,light_type,lights,normal,srgb", BWD_CASES)
def test_backward_map_gradients_guarded(dt, workflow, light_type, lights, normal, srgb):
    N, lib = _lib()
    i = BWD_CASES.index((dt, workflow, light_type, lights, normal, srgb))
    dtype = torch.float16 if dt == "f16" else torch.float32
    W = WIDTHS[(i * 7) % len(WIDTHS)]
    if dt == "f16" and lights == 1 and i % 3 == 0:
        W = 128 if i % 2 else 256                                   # the streamed kernel
    B, H = 1 + i % 3, 2 + i % 4
    y0, Ht = (i % 3, H + 5) if i % 2 else (0, None)                 # row bands of a taller map
    g = torch.Generator().manual_seed(1000 + i)
    maps = _material(g, B, H, W, workflow, dtype, normal)
    kw = _params(light_type, lights, srgb, workflow)
    kw.update(y_offset=y0, height_total=Ht)
    wt = torch.rand(B, 3, H, W, generator=g) - 0.35
    leaves = _leaves64(maps)
    ref = _render64(leaves, workflow, kw, y_offset=y0, H_total=Ht)
    (ref * wt.double()).sum().backward()
    present = [j for j, t in enumerate(maps) if t is not None]

    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    gout = gd.input(wt)
    results = {}
    for tuning in (None, {"max_vec": 1}):
        plan = _plan(views, kw, tuning=tuning)
        form = backward_form(plan.desc)
        tag = (dt, workflow, light_type, lights, normal, srgb, B, H, W, y0, tuning, form)
        streamed = dt == "f16" and lights == 1 and W % 128 == 0               # max_vec does not reach the streamed kernel
        assert form == ("stream" if streamed else ("one-pixel" if tuning or W < 4 else "vector")), tag
        outs = [None if t is None else gd.output(t.shape, dtype) for t in maps]
        _launch_backward(plan, gout, outs)
        gd.check(tag)
        for j in present:
            close64(outs[j], leaves[j].grad, tag + (j,), f16=dtype == torch.float16)
        results[form] = outs
        if tuning is None:
            for j in present:                                      # each gradient alone, NULL for every other one: the same values
                one = Guards()
                alone = [None] * 5
                alone[j] = one.output(maps[j].shape, dtype)
                _launch_backward(plan, gout, alone)
                one.check(tag + ("alone", j))
                assert torch.equal(alone[j], outs[j]), tag + ("alone", j)
            if form == "stream":                                   # bit-identical to the one-tile kernels at every run length
                for run in (0, 1, 7, 1000):
                    plan.set_tuning(bwd_run=run)
                    again = [None if t is None else gd.output(t.shape, dtype) for t in maps]
                    _launch_backward(plan, gout, again)
                    gd.check(tag + (run,))
                    for j in present:
                        assert torch.equal(again[j], outs[j]), tag + (run, j)


@pytest.mark.parametrize("workflow", WORKFLOWS)
@pytest.mark.parametrize("light_type", ["point", "directional"])
@pytest.mark.parametrize("full", [True, False])
def test_streamed_backward_guarded(workflow, light_type, full):
    """The streamed fp16 kernel: the "full" instantiation (every flag on, every gradient wanted) and the partial-store one (a subset of the
    gradients), run lengths 1 / 7 / 1000, a batch, guarded; bit-identical to the one-tile kernels (bwd_run 0), which are held to float64."""
    N, lib = _lib()
    g = torch.Generator().manual_seed(77 + WORKFLOWS.index(workflow) + (10 if full else 0))
    B, H, W = 2, 3, 256
    maps = _material(g, B, H, W, workflow, torch.float16)
    kw = _params(light_type, 1, True, workflow)
    wt = torch.rand(B, 3, H, W, generator=g) - 0.35
    leaves = _leaves64(maps)
    (_render64(leaves, workflow, kw) * wt.double()).sum().backward()
    wanted = [t is not None and (full or j in (0, 2)) for j, t in enumerate(maps)]
    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    gout = gd.input(wt)
    plan = _plan(views, kw)
    got = {}
    for run in (0, 1, 7, 1000):
        plan.set_tuning(bwd_run=run)
        assert backward_form(plan.desc) == ("stream" if run else "vector")
        outs = [gd.output(t.shape, torch.float16) if w else None for t, w in zip(maps, wanted)]
        _launch_backward(plan, gout, outs)
        gd.check((workflow, light_type, full, run))
        got[run] = outs
    for j, w in enumerate(wanted):
        if w:
            close64(got[0][j], leaves[j].grad, (workflow, light_type, j), f16=True)
            for run in (1, 7, 1000):
                assert torch.equal(got[run][j], got[0][j]), (workflow, light_type, full, run, j)


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("hw,tile,lights", [((5, 8), (2, 3), 1), ((4, 6), (3, 2), 3), ((3, 3), (2, 2), 1), ((6, 12), (2, 2), 1)])
def test_backward_of_tiled_descriptors_output_sized_guarded(dt, hw, tile, lights):
    """Tiled descriptors hand pbr_cook_torrance_backward OUTPUT-sized gradients (one value per output pixel; the fold is the caller's)."""
    dtype = torch.float16 if dt == "f16" else torch.float32
    (h, w), (ny, nx) = hw, tile
    g = torch.Generator().manual_seed(h * 31 + w + lights)
    B, H, W = 2, ny * h, nx * w
    y0, rows = 1, H - 2
    maps = _material(g, B, h, w, "metallic", dtype)
    kw = _params("point", lights)
    wt = torch.rand(B, 3, rows, W, generator=g) - 0.35
    rep = [t.double().repeat(1, 1, ny, nx)[:, :, y0:y0 + rows].requires_grad_(True) if t is not None else None for t in maps]
    (_render64(rep, "metallic", kw, y_offset=y0, H_total=H) * wt.double()).sum().backward()
    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    gout = gd.input(wt)
    plan = _plan(views, kw, tile=tile, y_offset=y0, rows=rows)
    assert plan.desc.map_height == h and plan.desc.height == rows and backward_form(plan.desc) in ("vector", "one-pixel")
    outs = [None if t is None else gd.output((B, t.shape[1], rows, W), dtype) for t in maps]
    _launch_backward(plan, gout, outs)
    gd.check((dt, hw, tile, lights))
    for o, r in zip(outs, rep):
        if o is not None:
            close64(o, r.grad, (dt, hw, tile, lights), f16=dtype == torch.float16)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. pbr_cook_torrance_backward_params: the workspace promise "whatever the tuning knobs say"

KNOBS = [dict(block_log2=b, max_vec=v, scalar_base=s) for b in (6, 7, 8) for v in (1, 4, 8) for s in (0, 2)]


@pytest.mark.parametrize("light_type", ["point", "directional"])
@pytest.mark.parametrize("lights", [1, 3])
@pytest.mark.parametrize("W", [8, 7, 130, 5])
def test_param_gradients_exact_workspace_every_knob(light_type, lights, W):
    N, lib = _lib()
    g = torch.Generator().manual_seed(500 + W + lights)
    B, H = (2, 5) if W < 100 else (1, 3)
    maps = _material(g, B, H, W, "metallic")
    kw = _params(light_type, lights)
    wt = torch.rand(B, 3, H, W, generator=g) - 0.35
    leaves = _leaves64(maps)
    view = torch.tensor(kw["view_dir"], dtype=torch.float64, requires_grad=True)
    lt = torch.tensor(kw["light"], dtype=torch.float64, requires_grad=True)
    it = torch.tensor(kw["light_intensity"], dtype=torch.float64, requires_grad=True)
    (_render64(leaves, "metallic", kw, view=view, lights=lt, intens=it) * wt.double()).sum().backward()
    want = torch.cat([view.grad, lt.grad.reshape(-1), it.grad.reshape(-1)])
    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    gout = gd.input(wt)
    plan = _plan(views, kw)
    nbytes = lib.pbr_param_grad_workspace_bytes(ctypes.byref(plan.desc))      # under the rules
    assert nbytes > 0
    first = {}
    for knobs in KNOBS:
        plan.set_tuning(**knobs)
        assert lib.pbr_param_grad_workspace_bytes(ctypes.byref(plan.desc)) == nbytes, knobs     # the knobs never grow the promise
        tag = (light_type, lights, W, knobs, backward_form(plan.desc, with_params=True))
        ws = gd.workspace(nbytes)
        gp = gd.output((3 + 6 * lights,))
        outs = [None if t is None else gd.output(t.shape) for t in maps]
        N.check(lib.pbr_cook_torrance_backward_params(ctypes.byref(plan.desc), P(gout), *[P(t) for t in outs], P(gp), P(ws), _stream()))
        gd.check(tag)
        close64(gp, want, tag, scale=True)
        for o, l in zip(outs, leaves):
            if o is not None:
                close64(o, l.grad, tag)
        # the same pixels per lane under every other knob: the same fixed-order sums, bit for bit
        first.setdefault(tag[-1], gp.clone())
        assert torch.equal(gp, first[tag[-1]]), tag


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. pbr_cook_torrance_mse_step: one-tile, streamed, several lights, tiled; the loss a guarded float, the workspace exact

MSE_CASES = {
    "one-tile f32": dict(dt="f32", lights=1, W=37, H=5, B=2),
    "one-tile even f32": dict(dt="f32", lights=1, W=130, H=3, B=1),
    "streamed f16": dict(dt="f16", lights=1, W=256, H=3, B=2),
    "one-tile f16": dict(dt="f16", lights=1, W=256, H=3, B=2, tuning=dict(mse_stream=0)),
    "several lights": dict(dt="f32", lights=3, W=20, H=6, B=3),
    "tiled": dict(dt="f32", lights=1, W=8, H=5, B=2, tile=(2, 3)),
    "tiled f16": dict(dt="f16", lights=1, W=12, H=3, B=1, tile=(3, 2)),
    "many workgroups": dict(dt="f32", lights=1, W=64, H=300, B=1),
}


@pytest.mark.parametrize("case", list(MSE_CASES))
def test_loss_step_exact_workspace_and_guarded_loss(case):
    N, lib = _lib()
    c = MSE_CASES[case]
    dtype = torch.float16 if c["dt"] == "f16" else torch.float32
    g = torch.Generator().manual_seed(len(case) * 13 + c["W"])
    B, H, W = c["B"], c["H"], c["W"]
    ny, nx = c.get("tile", (1, 1))
    maps = _material(g, B, H, W, "metallic", dtype)
    kw = _params("point", c["lights"])
    target = torch.rand(B, 3, ny * H, nx * W, generator=g)
    leaves = _leaves64(maps)
    img = _render64([None if t is None else t.repeat(1, 1, ny, nx) for t in leaves], "metallic", kw)
    loss64 = ((img - target.double()) ** 2).mean()
    loss64.backward()
    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    tgt = gd.input(target)
    extra = dict(tile=(ny, nx)) if (ny, nx) != (1, 1) else {}
    plan = _plan(views, kw, **extra)
    nbytes = lib.pbr_mse_step_workspace_bytes(ctypes.byref(plan.desc))
    assert nbytes > 0, case
    tiled = bool(extra)
    streamed = not tiled and dtype == torch.float16 and c["lights"] == 1 and W % 128 == 0 and c.get("tuning", {}).get("mse_stream", 1) != 0
    assert case.startswith("streamed") == streamed and case.startswith("tiled") == tiled
    first = None
    for knobs in [c.get("tuning", {})] + ([] if tiled else [dict(k, **c.get("tuning", {})) for k in KNOBS]):
        if knobs:
            plan.set_tuning(**knobs)
        tag = (case, knobs)
        ws = gd.workspace(nbytes)
        loss = gd.output((1,))
        outs = [None if t is None else gd.output(t.shape, dtype) for t in maps]
        N.check(lib.pbr_cook_torrance_mse_step(ctypes.byref(plan.desc), P(tgt), *[P(t) for t in outs], P(loss), P(ws), _stream()))
        gd.check(tag)
        assert abs(float(loss) - float(loss64.detach())) <= 2e-6 * float(loss64.detach()), (tag, float(loss), float(loss64.detach()))
        for o, l in zip(outs, leaves):
            if o is not None:
                close64(o, l.grad, tag, rel=2e-5, f16=dtype == torch.float16, scale=True)
        if first is None:
            first = outs
        elif knobs.get("max_vec", 8) != 1 or W % 2:
            for x, y in zip(outs, first):
                assert x is None or torch.equal(x, y), tag


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. pbr_cook_torrance_backward_folded, two-kernel form (map rows shorter than one 4-texel lane: the repeat-inner walk takes every other width)


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("hw,tile,lights,band", [((5, 3), (2, 3), 1, None), ((4, 2), (3, 2), 2, None), ((3, 3), (2, 2), 1, None),
                                                 ((6, 1), (2, 5), 1, None), ((2, 2), (3, 3), 3, None)])
def test_folded_backward_two_kernel_form_exact_workspace(dt, hw, tile, lights, band):
    N, lib = _lib()
    dtype = torch.float16 if dt == "f16" else torch.float32
    (h, w), (ny, nx) = hw, tile
    g = torch.Generator().manual_seed(h * 100 + w * 10 + lights)
    B, H, W = 2, ny * h, nx * w
    y0, rows = band or (0, H)
    maps = _material(g, B, h, w, "metallic", dtype)
    kw = _params("point", lights)
    wt = torch.rand(B, 3, rows, W, generator=g) - 0.35
    leaves = _leaves64(maps)
    img = _render64([None if t is None else t.repeat(1, 1, ny, nx) for t in leaves], "metallic", kw)
    (img[:, :, y0:y0 + rows] * wt.double()).sum().backward()
    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    gout = gd.input(wt)
    plan = _plan(views, kw, tile=tile, y_offset=y0, rows=rows)
    nbytes = lib.pbr_backward_folded_workspace_bytes(ctypes.byref(plan.desc))
    assert nbytes > 0, (dt, hw, tile)                              # the two-kernel form: backward into the workspace, then the fold
    ws = gd.workspace(nbytes)
    outs = [None if t is None else gd.output(t.shape, dtype) for t in maps]
    N.check(lib.pbr_cook_torrance_backward_folded(ctypes.byref(plan.desc), P(gout), *[P(t) for t in outs], P(ws), _stream()))
    gd.check((dt, hw, tile, lights, band))
    for o, l in zip(outs, leaves):
        if o is not None:
            # fp16: the two-kernel form rounds every repeat's gradient before the fold sums them
            close64(o, l.grad, (dt, hw, tile, lights, band), rel=2e-5 if dt == "f32" else 2e-3, scale=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. blend: pbr_blend_normal_sign, pbr_cook_torrance_blend, pbr_cook_torrance_blend_backward


def _blend_setup(gd, g, B, H, W, workflow, shared_mask, flat=False):
    from test_gpu_blend_backward import _material as bmat
    m1 = [bmat(g, H, W, workflow, flat) for _ in range(B)]
    m2 = [bmat(g, H, W, workflow, flat) for _ in range(B)]
    masks = [torch.rand(1, H, W, generator=g)] * (1 if shared_mask else B)
    masks = masks * B if shared_mask else masks
    key = "specular" if workflow == "specular" else "metallic"
    names = ("albedo", "normal", "roughness", key)
    stack = lambda ms: {k: torch.stack([m[k] for m in ms]) for k in names}
    s1, s2 = stack(m1), stack(m2)
    v1 = {k: gd.input(t) for k, t in s1.items()}
    v2 = {k: gd.input(t) for k, t in s2.items()}
    vm = gd.input(masks[0][None] if shared_mask else torch.stack(masks))

    return m1, m2, masks, v1, v2, vm


@pytest.mark.parametrize("workflow", WORKFLOWS)
@pytest.mark.parametrize("light_type", ["point", "directional"])
@pytest.mark.parametrize("sign_mode,shared_mask,W", [("compute", False, 46), ("compute", True, 5), ("given", False, 8), ("given", True, 130)])
def test_blend_forward_and_backward_guarded(workflow, light_type, sign_mode, shared_mask, W):
    from pypbr_amd import functional as F
    from test_gpu_blend_backward import _reference_grads
    N, lib = _lib()
    g = torch.Generator().manual_seed(W * 3 + WORKFLOWS.index(workflow) + (5 if shared_mask else 0))
    B, H = 2, 4
    gd = Guards()
    m1, m2, masks, v1, v2, vm = _blend_setup(gd, g, B, H, W, workflow, shared_mask, flat=(W == 8))
    kw = _params(light_type, 1, True, workflow)
    kw.pop("albedo_is_srgb"); kw.pop("specular_is_srgb"); kw.pop("return_srgb")
    key = "specular" if workflow == "specular" else "metallic"
    wt = torch.rand(B, 3, H, W, generator=g) - 0.4
    given = sign_mode == "given"
    flags = gd.output((B,), torch.int32, init=torch.zeros(B, dtype=torch.int32)) if given else gd.workspace(4 * B)
    out = gd.output((B, 3, H, W))
    plan = _plan([v1["albedo"], v1["normal"], v1["roughness"], v1.get("metallic"), v1.get("specular")], kw, out=out,
                 blend=(v2["albedo"], v2["normal"], v2["roughness"], v2.get("metallic"), v2.get("specular"), vm))
    blend = plan._blend
    st = _stream()
    if given:
        blend.sign_mode = N.BLEND_SIGN_GIVEN
        N.check(lib.pbr_blend_normal_sign(ctypes.byref(plan.desc), ctypes.byref(blend), P(flags), st))    # zeroed, then set: the header's recipe
    N.check(lib.pbr_cook_torrance_blend(ctypes.byref(plan.desc), ctypes.byref(blend), P(flags), st))
    gd.check(("forward", workflow, light_type, sign_mode, W))
    assert lib.pbr_blend_backward_serves(ctypes.byref(plan.desc)) == 1
    gout = gd.input(wt)
    pick = [("albedo", "roughness"), ("normal", key), ("albedo", "normal", "roughness", key)][(W + len(light_type)) % 3]
    g1 = {k: gd.output((B, CHANNELS[("albedo", "normal", "roughness", "metallic", "specular").index(k)], H, W)) for k in pick}
    g2 = {k: gd.output(t.shape) for k, t in v2.items()}
    gm = gd.output((B, 1, H, W))
    mg = lambda d: N.MapGrads(*[P(d.get(k)) for k in ("albedo", "normal", "roughness", "metallic", "specular")])
    G1, G2 = mg(g1), mg(g2)
    N.check(lib.pbr_cook_torrance_blend_backward(ctypes.byref(plan.desc), ctypes.byref(blend), P(flags), P(gout), ctypes.byref(G1),
                                                 ctypes.byref(G2), P(gm), st))
    tag = ("backward", workflow, light_type, sign_mode, shared_mask, W, pick)
    gd.check(tag)
    view, light, inten = (torch.tensor(kw["view_dir"]), torch.tensor(kw["light"][0]), torch.tensor(kw["light_intensity"][0]))
    for b in range(B):
        ref, r1, r2, rm = _reference_grads(m1[b], m2[b], masks[b], wt[b], view, light, inten, light_type, kw["light_size"],
                                           converted=(workflow == "converted"))
        assert (out[b].cpu().double() - ref).abs().max().item() <= 1e-5, tag + (b,)
        for k, t in g1.items():
            close64(t[b], r1[k].grad, tag + (b, 1, k))
        for k, t in g2.items():
            close64(t[b], r2[k].grad, tag + (b, 2, k))
        close64(gm[b], rm.grad, tag + (b, "mask"))


@pytest.mark.parametrize("hw,tile,band", [((6, 8), (2, 3), None), ((5, 12), (3, 2), (2, 9)), ((4, 4), (2, 2), (0, 5))])
def test_tiled_blend_backward_map_sized_guarded(hw, tile, band):
    from test_gpu_round6 import _reference_tiled
    N, lib = _lib()
    (h, w), (ny, nx) = hw, tile
    g = torch.Generator().manual_seed(h * 7 + w)
    gd = Guards()
    m1, m2, masks, v1, v2, vm = _blend_setup(gd, g, 1, h, w, "metallic", False)
    kw = _params("point", 1)
    kw.pop("albedo_is_srgb"); kw.pop("specular_is_srgb"); kw.pop("return_srgb"); kw.pop("convert_to_diffuse_specular")
    H, W = ny * h, nx * w
    y0, rows = band or (0, H)
    wt_full = torch.zeros(1, 3, H, W)
    wt_full[:, :, y0:y0 + rows] = torch.rand(1, 3, rows, W, generator=g) - 0.4
    flags = gd.workspace(4)
    plan = _plan([v1["albedo"], v1["normal"], v1["roughness"], v1["metallic"], None], kw, tile=tile, y_offset=y0, rows=rows,
                 blend=(v2["albedo"], v2["normal"], v2["roughness"], v2["metallic"], None, vm))
    assert plan.desc.map_height == h and lib.pbr_blend_backward_serves(ctypes.byref(plan.desc)) == 1, (hw, tile, band)
    st = _stream()
    gout = gd.input(wt_full[:, :, y0:y0 + rows].contiguous())
    g1 = {k: gd.output(t.shape) for k, t in v1.items()}
    g2 = {k: gd.output(t.shape) for k, t in v2.items()}
    gm = gd.output((1, 1, h, w))
    mg = lambda d: N.MapGrads(*[P(d.get(k)) for k in ("albedo", "normal", "roughness", "metallic", "specular")])
    G1, G2 = mg(g1), mg(g2)
    N.check(lib.pbr_cook_torrance_blend_backward(ctypes.byref(plan.desc), ctypes.byref(plan._blend), P(flags), P(gout), ctypes.byref(G1),
                                                 ctypes.byref(G2), P(gm), st))
    gd.check((hw, tile, band))
    ref, r1, r2, rm = _reference_tiled(m1[0], m2[0], masks[0], wt_full[0], torch.tensor(kw["view_dir"]), torch.tensor(kw["light"][0]),
                                       torch.tensor(kw["light_intensity"][0]), "point", kw["light_size"], tile)
    for k in g1:
        close64(g1[k][0], r1[k].grad, (hw, tile, band, 1, k))
        close64(g2[k][0], r2[k].grad, (hw, tile, band, 2, k))
    close64(gm[0], rm.grad, (hw, tile, band, "mask"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. forward gaps: every form with an fp32 and an fp16 result, written into a strided result whose gaps are guarded

FWD_FORMS = {
    # name suffix: (map dtype, lights, batch, width, tuning, tile)
    "_v1": ("f32", 1, 2, 13, dict(max_vec=1), None),
    "_v4": ("f32", 1, 2, 13, None, None),
    "_v4_multi": ("f32", 3, 3, 21, None, None),
    "_v8": ("f16", 1, 2, 24, None, None),
    "_v2_b2": ("f32", 2, 2, 12, None, None),
    "_v2_b4": ("f32", 3, 4, 7, None, None),
    "ctr_": ("f32", 1, 2, 12, None, (2, 3)),
}


@pytest.mark.parametrize("out_dt", ["f32", "f16"])
@pytest.mark.parametrize("form", list(FWD_FORMS))
def test_forward_forms_into_strided_guarded_results(form, out_dt):
    mdt, lights, B, w, tuning, tile = FWD_FORMS[form]
    dtype = torch.float16 if mdt == "f16" else torch.float32
    odtype = torch.float16 if out_dt == "f16" else torch.float32
    g = torch.Generator().manual_seed(list(FWD_FORMS).index(form) * 10 + len(out_dt))
    h = 5
    maps = _material(g, B, h, w, "metallic", dtype)
    kw = _params("point", lights)
    ny, nx = tile or (1, 1)
    H, W = ny * h, nx * w
    gd = Guards()
    views = [None if t is None else gd.input(t) for t in maps]
    # a strided result: 8 spare elements between channel planes, 24 between materials, all of it sentinel-filled
    cs = H * W + 8
    bs = 3 * cs + 24
    big = gd.output((B * bs,), odtype, init=torch.full((B * bs,), UNWRITTEN))
    out = big.as_strided((B, 3, H, W), (bs, cs, W, 1))
    extra = dict(tile=tile) if tile else {}
    plan = _plan(views, kw, out=out, tuning=tuning, **extra)
    name = plan.kernel_name
    assert (name.startswith("ctr_") if form == "ctr_" else name.endswith(form)) and ("_%s_%s_" % (mdt, out_dt)) in name, (form, name)
    assert (plan.desc.out_channel_stride, plan.desc.out_batch_stride) == (cs, bs)
    plan.launch()
    gd.check((form, out_dt, name))
    grid = torch.zeros(B * bs, dtype=torch.bool, device="cuda")
    grid.as_strided((B, 3, H, W), (bs, cs, W, 1)).fill_(True)
    assert bool((big[~grid] == UNWRITTEN).all()), ("a gap between planes or materials was written", form, out_dt, name)
    assert not bool((out == UNWRITTEN).any()), (form, out_dt, name)
    np_maps = [None if t is None else t.repeat(1, 1, ny, nx).double().numpy() for t in maps]
    ref = C.render(np_maps[0], np_maps[1], np_maps[2], np_maps[3], None, view=kw["view_dir"], lights=kw["light"], intensities=kw["light_intensity"],
                   light_type="point", light_size=kw["light_size"], workflow="metallic", dtype=np.float64)
    err = np.abs(out.float().cpu().numpy().astype(np.float64) - ref)
    bound = 1e-5 + (np.abs(ref) * 2.0 ** -11 if odtype == torch.float16 else 0.0)
    assert (err <= bound).all(), (form, out_dt, name, float(err.max()))


@pytest.mark.parametrize("W", [5, 7, 127, 130, 256, 36])
def test_fp16_results_of_ragged_rows_are_bit_identical_unguarded(W):
    """The overlapped last lane of a ragged row with 8-byte fp16 stores: the guarded, off-alignment and plain launches write the same halves."""
    g = torch.Generator().manual_seed(W)
    B, H = 2, 3
    maps = _material(g, B, H, W, "specular", torch.float16)
    kw = _params("directional", 1, workflow="specular")
    plain = _plan([None if t is None else t.cuda() for t in maps], kw, out_dtype=torch.float16)
    plain.launch()
    for gdist in (G, G + 1, G + 3):
        gd = Guards(gdist)
        views = [None if t is None else gd.input(t) for t in maps]
        out = gd.output((B, 3, H, W), torch.float16)
        plan = _plan(views, kw, out=out)
        plan.launch()
        gd.check((W, gdist, plan.kernel_name))
        if gdist == G:
            assert plan.kernel_name == plain.kernel_name
        assert torch.equal(out, plain.result) or gdist != G, (W, gdist)
        assert (out.float() - plain.result.float()).abs().max().item() <= 2e-3, (W, gdist, plan.kernel_name)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. stand-alone map kernels and their backward kernels

SIZES = (1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 257, 4097)
OFFSETS = (0, 1, 2, 3)


def _sweep():
    return [(n, o) for n in SIZES for o in OFFSETS if o == 0 or n in (5, 64, 257, 4097)]


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_colour_transfers_and_their_gradients_guarded(dt):
    N, lib = _lib()
    dtype = torch.float16 if dt == "f16" else torch.float32
    code = N.F16 if dt == "f16" else N.F32
    st = _stream()
    for n, off in _sweep():
        g = torch.Generator().manual_seed(n + off)
        x = torch.rand(n, generator=g).to(dtype)
        up = (torch.rand(n, generator=g) - 0.3).to(dtype)
        for name, fwd, bwd, ref in (("to_linear", lib.pbr_srgb_to_linear, lib.pbr_srgb_to_linear_backward, O.srgb_to_linear),
                                    ("to_srgb", lib.pbr_linear_to_srgb, lib.pbr_linear_to_srgb_backward, O.linear_to_srgb)):
            tag = (dt, n, off, name)
            gd = Guards(G + off)
            src, gout = gd.input(x), gd.input(up)
            dst, gin = gd.output((n,), dtype), gd.output((n,), dtype)
            N.check(fwd(P(src), P(dst), n, code, st))
            N.check(bwd(P(src), P(gout), P(gin), n, code, st))
            gd.check(tag)
            x64 = x.double().requires_grad_(True)
            y64 = ref(x64)
            (y64 * up.double()).sum().backward()
            close64(dst, y64.detach(), tag, rel=2e-6 if dt == "f32" else 1e-3)
            close64(gin, x64.grad, tag, rel=2e-5 if dt == "f32" else 1e-3, f16=dt == "f16")
            inplace = Guards(G + off)                             # dst == src
            buf = inplace.output((n,), dtype, init=x)
            N.check(fwd(P(buf), P(buf), n, code, st))
            inplace.check(tag + ("in place",))
            assert torch.equal(buf, dst), tag


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("srgb", [True, False])
def test_material_conversions_and_their_gradients_guarded(dt, srgb):
    N, lib = _lib()
    dtype = torch.float16 if dt == "f16" else torch.float32
    code = N.F16 if dt == "f16" else N.F32
    st = _stream()
    tol = dict(rel=2e-5) if dt == "f32" else dict(rel=1e-3, f16=True)
    pooled = [0, 0]                                               # decided elements / elements of the to_basecolor_metallic gradients, over the sweep
    for n, off in _sweep():
        g = torch.Generator().manual_seed(n * 3 + off)
        B = 2 if n % 2 else 1
        a, m = torch.rand(B, 3, n, generator=g).to(dtype), torch.rand(B, 1, n, generator=g).to(dtype)
        gdf, gsp = (torch.rand(B, 3, n, generator=g) - 0.4).to(dtype), (torch.rand(B, 3, n, generator=g) - 0.4).to(dtype)
        tag = (dt, srgb, n, off, B)
        a64, m64 = a.double().requires_grad_(True), m.double().requires_grad_(True)
        dif64, spe64 = O.metallic_to_diffuse_specular(O.srgb_to_linear(a64) if srgb else a64, m64)
        gd = Guards(G + off)
        va, vm, vgd, vgs = gd.input(a), gd.input(m), gd.input(gdf), gd.input(gsp)
        dif, spe = gd.output((B, 3, n), dtype), gd.output((B, 3, n), dtype)
        N.check(lib.pbr_metallic_to_specular(P(va), P(vm), P(dif), P(spe), B, n, int(srgb), code, st))
        for which in ("both", "no diffuse", "no specular"):
            ga, gm = gd.output((B, 3, n), dtype), gd.output((B, 1, n), dtype)
            N.check(lib.pbr_metallic_to_specular_backward(P(va), P(vm), None if which == "no diffuse" else P(vgd),
                                                          None if which == "no specular" else P(vgs), P(ga), P(gm), B, n, int(srgb), code, st))
            gd.check(tag + (which,))
            a64.grad = m64.grad = None
            ((dif64 * gdf.double()) * (which != "no diffuse") + (spe64 * gsp.double()) * (which != "no specular")).sum().backward(retain_graph=True)
            close64(ga, a64.grad, tag + (which, "albedo"), **tol)
            close64(gm, m64.grad, tag + (which, "metallic"), **tol)
        close64(dif, dif64.detach(), tag, **tol)
        close64(spe, spe64.detach(), tag, **tol)
        one = Guards(G + off)                                     # NULL results: only the one asked for is written
        va2, vm2, vgd2 = one.input(a), one.input(m), one.input(gdf)
        ga2 = one.output((B, 3, n), dtype)
        N.check(lib.pbr_metallic_to_specular_backward(P(va2), P(vm2), P(vgd2), None, P(ga2), None, B, n, int(srgb), code, st))
        one.check(tag + ("albedo only",))
        # diffuse/specular -> basecolor/metallic and its backward
        d, s = torch.rand(3 * n, generator=g).to(dtype), torch.rand(3 * n, generator=g).to(dtype)
        gb, gmm = (torch.rand(3 * n, generator=g) - 0.4).to(dtype), (torch.rand(3 * n, generator=g) - 0.4).to(dtype)
        gd2 = Guards(G + off)
        vd, vs, vgb, vgm = gd2.input(d), gd2.input(s), gd2.input(gb), gd2.input(gmm)
        bc, mt = gd2.output((3 * n,), dtype), gd2.output((3 * n,), dtype)
        gdd, gss = gd2.output((3 * n,), dtype), gd2.output((3 * n,), dtype)
        N.check(lib.pbr_specular_to_metallic(P(vd), P(vs), P(bc), P(mt), 3 * n, int(srgb), code, st))
        N.check(lib.pbr_specular_to_metallic_backward(P(vd), P(vs), P(vgb), P(vgm), P(gdd), P(gss), 3 * n, int(srgb), code, st))
        gd2.check(tag + ("to metallic",))
        # the thresholded selects of diffuse.py:136-144 are re-taken with fp32 arithmetic: the fp32 C oracle, not float64, decides the branches
        d_np = C.srgb_to_linear(d.float().numpy()) if srgb else d.float().numpy()
        bc_ref, mt_ref = C.specular_to_metallic(d_np.reshape(3, 1, n), s.float().numpy().reshape(3, 1, n))     # [3][P] planes
        close64(bc, torch.from_numpy(bc_ref).reshape(-1), tag + ("basecolor",), rel=1e-5, f16=dt == "f16")
        close64(mt, torch.from_numpy(mt_ref).reshape(-1), tag + ("metallic",), rel=1e-5, f16=dt == "f16")
        # the gradients, against float64 autograd of the oracle, on the elements the map-op fixture's rule calls decided (every compared
        # quantity 1e-3 from its threshold, the oracle's own float32 gradient within half the band, |den| >= 0.02 on live elements)
        d64, s64 = d.double().requires_grad_(True), s.double().requires_grad_(True)
        b64, t64 = O.diffuse_specular_to_basecolor_metallic(O.srgb_to_linear(d64) if srgb else d64, s64)
        ((b64 * gb.double()).sum() + (t64 * gmm.double()).sum()).backward()
        keep = MC.decided_to_basecolor_metallic(d.double(), s.double(), srgb, gb.double(), gmm.double())
        pooled[0] += int(keep.sum())
        pooled[1] += keep.numel()
        assert bool(torch.isfinite(gdd.float()).all()) and bool(torch.isfinite(gss.float()).all()), tag
        if bool(keep.any()):
            close64(gdd.cpu()[keep], d64.grad[keep], tag + ("g diffuse",), **tol)
            close64(gss.cpu()[keep], s64.grad[keep], tag + ("g specular",), **tol)
    print("to_basecolor_metallic gradients %s srgb=%s: %.1f %% of %d elements decided and compared" % (dt, srgb, 100.0 * pooled[0] / pooled[1], pooled[1]))


def test_decode_normal_and_its_gradient_guarded():
    N, lib = _lib()
    st = _stream()
    for n, off in _sweep():
        for channels in (2, 3):
            for signed in ((False, True) if channels == 3 else (False,)):
                g = torch.Generator().manual_seed(n * 7 + off + channels)
                # 2 channels: x, y in [-0.5, 0.5] keep z = sqrt(1 - x^2 - y^2) away from its clamp, where the gradient has no scale
                x = torch.rand(channels, n, generator=g) * (0.8 if channels == 3 else 0.5) + (0.1 if channels == 3 else 0.25)
                if signed and channels == 3:
                    x[0, n // 2] = -0.25                            # "already signed": kept as it is
                up = torch.rand(3, n, generator=g) - 0.4
                tag = (n, off, channels, signed)
                gd = Guards(G + off)
                src, gout = gd.input(x), gd.input(up)
                dst = gd.output((3, n))
                flag = gd.workspace(4)
                gin = gd.output((channels, n))
                N.check(lib.pbr_decode_normal(P(src), P(dst), channels, n, N.F32, P(flag), st))
                N.check(lib.pbr_decode_normal_backward(P(src), P(gout), P(gin), channels, n, P(flag), st))
                gd.check(tag)
                x64 = x.double().requires_grad_(True)
                y64 = O.decode_normal(x64)
                (y64 * up.double()).sum().backward()
                close64(dst, y64.detach(), tag, rel=1e-5)             # 2 channels: z = sqrt(1 - x^2 - y^2) near its clamp
                close64(gin, x64.grad, tag)
                if channels == 3:                                  # dst == src
                    inplace = Guards(G + off)
                    buf = inplace.output((3, n), init=x)
                    flag2 = inplace.workspace(4)
                    N.check(lib.pbr_decode_normal(P(buf), P(buf), 3, n, N.F32, P(flag2), st))
                    inplace.check(tag + ("in place",))
                    assert torch.equal(buf, dst), tag


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_fold_gradient_guarded(dt):
    N, lib = _lib()
    dtype = torch.float16 if dt == "f16" else torch.float32
    st = _stream()
    for (B, C_, h, w, ny, nx, fold_batch) in ((1, 1, 1, 1, 2, 3, 0), (2, 3, 3, 5, 2, 2, 1), (3, 1, 4, 7, 1, 3, 0), (2, 3, 2, 64, 3, 1, 1),
                                              (1, 3, 9, 130, 2, 2, 0), (4, 1, 3, 3, 3, 3, 1)):
        g = torch.Generator().manual_seed(B * 100 + w)
        src = (torch.rand(B, C_, ny * h, nx * w, generator=g) - 0.4).to(dtype)
        want = src.double().reshape(B, C_, ny, h, nx, w).sum((2, 4))
        if fold_batch:
            want = want.sum(0, keepdim=True)
        tag = (dt, B, C_, h, w, ny, nx, fold_batch)
        gd = Guards()
        vs = gd.input(src)
        dst = gd.output(tuple(want.shape), dtype)
        N.check(lib.pbr_fold_gradient_typed(P(vs), P(dst), B, C_, h, w, ny, nx, fold_batch, N.F16 if dt == "f16" else N.F32, st))
        if dt == "f32":
            dst2 = gd.output(tuple(want.shape))
            N.check(lib.pbr_fold_gradient(P(vs), P(dst2), B, C_, h, w, ny, nx, fold_batch, st))
        gd.check(tag)
        close64(dst, want, tag, rel=1e-5 if dt == "f32" else 2e-3, scale=True)
        if dt == "f32":
            assert torch.equal(dst, dst2), tag


def test_blend_maps_masks_and_their_gradients_guarded():
    N, lib = _lib()
    st = _stream()
    for n, off in _sweep():
        for channels, is_normal in ((1, 0), (3, 0), (3, 1)):
            g = torch.Generator().manual_seed(n * 5 + off + channels + is_normal)
            if is_normal:
                m1 = torch.cat([torch.rand(2, n, generator=g) - 0.5, torch.ones(1, n)], 0)
                m2 = torch.cat([torch.rand(2, n, generator=g) - 0.5, torch.ones(1, n)], 0)
            else:
                m1, m2 = torch.rand(channels, n, generator=g), torch.rand(channels, n, generator=g)
            mask, up = torch.rand(n, generator=g), torch.rand(channels, n, generator=g) - 0.4
            prior = torch.rand(n, generator=g)
            tag = (n, off, channels, is_normal)
            gd = Guards(G + off)
            v1, v2, vm, vu = gd.input(m1), gd.input(m2), gd.input(mask), gd.input(up)
            out = gd.output((channels, n))
            g1, g2, gm = gd.output((channels, n)), gd.output((channels, n)), gd.output((n,))
            gacc = gd.output((n,), init=prior)                        # accumulate_mask: g_mask += ...
            N.check(lib.pbr_blend_maps(P(v1), P(v2), P(vm), P(out), channels, n, is_normal, st))
            N.check(lib.pbr_blend_maps_backward(P(v1), P(v2), P(vm), P(vu), P(g1), P(g2), P(gm), channels, n, is_normal, 0, st))
            N.check(lib.pbr_blend_maps_backward(P(v1), P(v2), P(vm), P(vu), None, None, P(gacc), channels, n, is_normal, 1, st))
            gd.check(tag)
            r1, r2, rm = m1.double().requires_grad_(True), m2.double().requires_grad_(True), mask.double().requires_grad_(True)
            ref = BO.blend_normals(r1, r2, rm[None]) if is_normal else BO.blend_maps(r1, r2, rm[None])
            (ref * up.double()).sum().backward()
            close64(out, ref.detach(), tag, rel=2e-6)
            close64(g1, r1.grad, tag + ("map1",))
            close64(g2, r2.grad, tag + ("map2",))
            close64(gm, rm.grad, tag + ("mask",))
            close64(gacc, rm.grad + prior.double(), tag + ("accumulated mask",))
        # the sigmoid mask and its backward, the gradient mask
        g = torch.Generator().manual_seed(n + off)
        p1, p2, up = torch.rand(n, generator=g), torch.rand(n, generator=g), torch.rand(n, generator=g) - 0.4
        gd = Guards(G + off)
        v1, v2, vu = gd.input(p1), gd.input(p2), gd.input(up)
        mask = gd.output((n,))
        N.check(lib.pbr_blend_sigmoid_mask(P(v1), P(v2), P(mask), n, 0.05, 0.1, st))
        torch.cuda.synchronize()
        vmask = gd.input(mask.clone())
        gp1, gp2 = gd.output((n,)), gd.output((n,))
        N.check(lib.pbr_blend_sigmoid_mask_backward(P(vmask), P(vu), P(gp1), P(gp2), n, 0.1, st))
        gd.check((n, off, "sigmoid"))
        r1, r2 = p1.double().requires_grad_(True), p2.double().requires_grad_(True)
        ref = BO.sigmoid_mask(r1, r2, 0.1, 0.05)
        (ref * up.double()).sum().backward()
        close64(mask, ref.detach(), (n, off, "sigmoid"), rel=2e-6)
        close64(gp1, r1.grad, (n, off, "sigmoid grad 1"), scale=True)
        close64(gp2, r2.grad, (n, off, "sigmoid grad 2"), scale=True)
    for h, w in ((1, 1), (3, 5), (7, 64), (2, 257), (33, 9)):
        for vertical in (0, 1):
            gd = Guards()
            mask = gd.output((1, h, w))
            N.check(lib.pbr_blend_gradient_mask(P(mask), h, w, vertical, _stream()))
            gd.check((h, w, vertical))
            close64(mask, BO.gradient_mask(h, w, "vertical" if vertical else "horizontal").double(), (h, w, vertical), rel=1e-6)


def test_scale_by_device_scalar_guarded():
    N, lib = _lib()
    st = _stream()
    for dt in ("f32", "f16"):
        dtype = torch.float16 if dt == "f16" else torch.float32
        code = N.F16 if dt == "f16" else N.F32
        for n, off in _sweep():
            g = torch.Generator().manual_seed(n + off)
            x = (torch.rand(n, generator=g) - 0.5).to(dtype)
            gd = Guards(G + off)
            scalar = gd.input(torch.tensor([0.75]))
            buf = gd.output((n,), dtype, init=x)
            N.check(lib.pbr_scale_by_device_scalar(P(buf), n, code, P(scalar), st))
            gd.check((dt, n, off))
            assert torch.equal(buf.cpu(), (x.float() * 0.75).to(dtype)), (dt, n, off)
        gd = Guards(G + 1)
        xs = [(torch.rand(n, generator=g) - 0.5).to(dtype) for n in (1, 7, 64, 257, 4097)]
        bufs = [gd.output((x.numel(),), dtype, init=x) for x in xs]
        scalar = gd.input(torch.tensor([-1.5]))
        ptrs = (ctypes.c_void_p * 5)(*[P(b) for b in bufs])
        ns = (ctypes.c_size_t * 5)(*[x.numel() for x in xs])
        N.check(lib.pbr_scale_list_by_device_scalar(ptrs, ns, 5, code, P(scalar), st))
        gd.check((dt, "list"))
        for b, x in zip(bufs, xs):
            assert torch.equal(b.cpu(), (x.float() * -1.5).to(dtype)), dt


def test_unpack_image_guarded():
    N, lib = _lib()
    st = _stream()
    for bits in (8, 16):
        for (h, w, channels) in ((1, 1, 1), (3, 5, 3), (7, 9, 4), (4, 130, 2), (2, 257, 3)):
            for decode in ((0, 1) if channels in (2, 3) else (0,)):
                for layout in ("hwc", "chw_padded"):
                    g = torch.Generator().manual_seed(bits + h * w + channels)
                    hi = 256 if bits == 8 else 65536
                    vals = torch.randint(0, hi, (h, w, channels), generator=g)
                    if layout == "hwc":
                        store = vals
                        sc, sh, sw = 1, w * channels, channels
                    else:                                          # planar with 3 spare samples per row
                        store = torch.zeros(channels, h, w + 3, dtype=torch.int64)
                        store[:, :, :w] = vals.permute(2, 0, 1)
                        sc, sh, sw = h * (w + 3), w + 3, 1
                    raw = store.to(torch.uint8) if bits == 8 else (store.to(torch.int32) - 65536 * (store >= 32768).to(torch.int32)).to(torch.int16)
                    gd = Guards(G + 1)
                    src = gd.input(raw)
                    out_c = 3 if decode else channels
                    dst = gd.output((out_c, h, w))
                    N.check(lib.pbr_unpack_image(P(src), bits, channels, h, w, sc, sh, sw, P(dst), decode, st))
                    tag = (bits, h, w, channels, decode, layout)
                    gd.check(tag)
                    f = (vals.permute(2, 0, 1).double() / (hi - 1))
                    want = O.decode_normal(f.float()).double() if decode else f
                    close64(dst, want, tag, rel=2e-7 if not decode else 2e-6)


def test_prepare_device_params_exact_block():
    N, lib = _lib()
    from pypbr_amd import functional as F
    nbytes = lib.pbr_device_params_bytes()
    g = torch.Generator().manual_seed(5)
    for light_type in ("point", "directional"):
        for lights in (1, 3, 16):
            maps = _material(g, 1, 4, 8, "metallic")
            kw = _params(light_type, min(lights, 3))
            lt = torch.rand(lights, 3, generator=g) + 0.1
            it = torch.rand(lights, 3, generator=g)
            kw.update(light=lt.tolist(), light_intensity=it.tolist())
            plan = _plan([None if t is None else t.cuda() for t in maps], kw)
            want = plan.launch().clone()
            gd = Guards()
            block = gd.workspace(nbytes)
            vv, vl, vi = gd.input(torch.tensor(kw["view_dir"])), gd.input(lt), gd.input(it)
            N.check(lib.pbr_prepare_device_params(ctypes.byref(plan.desc), P(vv), P(vl), P(vi), lights, P(block), _stream()))
            gd.check((light_type, lights))
            plan.desc.device_params = P(block)
            got = plan.launch()
            torch.cuda.synchronize()
            assert (got - want).abs().max().item() <= 2e-6, (light_type, lights, float((got - want).abs().max()))
            plan.desc.device_params = None


# ---------------------------------------------------------------------------------------------------------------------------------------
# resize and its backward: every form pbr_resize_form reports, exact workspaces

RESIZE_SHAPES = [  # planes, h_in, w_in, h_out, w_out, antialias, knob PBR_TUNE_RESIZE_UP2, the family pbr_resize_form must report
    (2, 40, 52, 90, 101, 0, 1, "TWO_TAP"), (1, 33, 47, 80, 96, 1, 1, "TWO_TAP"),
    (3, 64, 96, 32, 48, 1, 1, "BAND_WALK"), (1, 128, 64, 16, 8, 1, 1, "BAND_WALK"),
    (1, 512, 520, 60, 70, 1, 1, "ROW_WALK"), (2, 300, 512, 40, 60, 1, 2, "ROW_WALK"),
    (2, 100, 130, 70, 60, 0, 1, "STRIP"), (1, 100, 200, 90, 150, 1, 0, "STRIP"), (3, 17, 5, 9, 3, 1, 1, "STRIP"),
    (1, 1024, 512, 20, 10, 1, 1, "TWO_PASS"),
]


@pytest.mark.parametrize("shape", RESIZE_SHAPES)
def test_resize_and_its_backward_exact_workspaces(shape):
    N, lib = _lib()
    planes, hi, wi, ho, wo, aa, knob, family = shape
    g = torch.Generator().manual_seed(hi * wi + ho)
    x = torch.rand(planes, hi, wi, generator=g)
    up = torch.rand(planes, ho, wo, generator=g) - 0.4
    st = _stream()
    try:
        lib.pbr_set_tuning(N.TUNE_RESIZE_UP2, knob)
        gd = Guards()
        src, gout = gd.input(x), gd.input(up)
        out = gd.output((planes, ho, wo))
        ws = gd.workspace(lib.pbr_resize_workspace_bytes(planes, hi, wo))
        form = lib.pbr_resize_form(P(src), P(out), planes, hi, wi, ho, wo, aa, P(ws))
        N.check(lib.pbr_resize_bilinear(P(src), P(out), planes, hi, wi, ho, wo, aa, P(ws), st))
        gin = gd.output((planes, hi, wi))
        ws2 = gd.workspace(lib.pbr_resize_backward_workspace_bytes(planes, hi, wi, ho, wo))
        N.check(lib.pbr_resize_bilinear_backward(P(gout), P(gin), planes, hi, wi, ho, wo, aa, P(ws2), st))
        gd.check((shape, form))
    finally:
        lib.pbr_set_tuning(N.TUNE_RESIZE_UP2, -1)
    assert form == getattr(N, "RESIZE_" + family), (shape, form)
    x64 = x.double().requires_grad_(True)
    ref = torch.nn.functional.interpolate(x64[None], size=(ho, wo), mode="bilinear", align_corners=False, antialias=bool(aa))[0]
    (ref * up.double()).sum().backward()
    close64(out, ref.detach(), (shape, form), rel=1e-5)
    close64(gin, x64.grad, (shape, form), rel=2e-5, scale=True)

