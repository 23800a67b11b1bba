"""Inputs that put render gradients on every branch of the reference's clamps, sRGB knees and sign tests.

TEST INFRASTRUCTURE ONLY (like torch_oracle.py): tests/test_branch_cases_host.py fixes the inputs on the CPU; the GPU
gradient tests of the backward kernels are to run on them.  No GPU code here.

The render backward (pypbr_amd/csrc/ct_backward.hpp) is a hand-written chain rule in which every clamp, knee and sign
test of cooktorrance.py is a select.  Random maps lit and seen from +Z never leave the ordinary branch of any of them.
The cases below are BUILT to leave it (angles from a grid, colours from a list, intensities per case), and `decisions`
says, from the float64 oracle alone, which side of which threshold every pixel is on:

    raw N.L, N.V and N.H of every light                         against 0
    stored albedo / specular channels that go through a decode  against 0, 0.04045 and 1
    every light's linear contribution, per channel              against 0 and 1
    several lights: the summed colour                           against 1
    return_srgb: the clamped colour                             against 0.0031308

A pixel is DECIDED when each of these is at least MARGIN = 1e-3 from its threshold -- 100 x the 1e-5 the forward is
asserted to, so an fp32 evaluation cannot be on the other side.  Two readings that the definition needs:

  * a light with N.L decided negative (N.L <= -MARGIN) contributes exactly 0 in any precision (radiance = clamp(N.L) = 0),
    so its contribution is not compared with 0 again (the gradient there is exactly 0);
  * `closed_ends`, and only that case, stores albedo channels of exactly 0.0 and 1.0 on purpose.  A stored value that
    EQUALS a clamp end is the same number in every precision: there it counts as decided, and whether the pixel is kept
    is settled by the agreement of the oracle's own float32 and float64 gradients (`well_conditioned`).

All map values are exactly representable in fp16, so fp16 and fp32 kernels and the float64 oracle see the same inputs.

STACK MODE (build(..., stack=True), STACK_ENTRY_CONFIGS; held by tests/test_light_stack_branches_host.py, run on the GPU by
tests/test_gpu_light_stack_branches.py): the same inputs read as a LIGHT STACK (csrc/ct_stack.hip) -- L images, image l being the
one-light evaluation for light l alone.  `render` gives [L,3,H,W], `gradients` differentiates the MSE over the stack (or sum(stack * W)),
and `decisions` lists one encode knee per light (that light's own clamped colour) and no summed colour.  `split_lights`, stack mode
only, puts three lights on different sides of the surface, so that the set of lit lights changes from pixel to pixel.

BLEND MODE (build_blend, BLEND_ENTRY_CONFIGS; held by tests/test_blend_branches_host.py, run on the GPU by tests/test_gpu_blend_branches.py):
two materials and a mask whose BLEND is the case, for the fused blend's backward (csrc/ct_blend_backward.hpp); see the section at the end.

CAMERA MODE (build(..., camera="fixed" | "per_shot"), CAMERA_ENTRY_CONFIGS; held by tests/test_camera_branches_host.py, run on the GPU by
tests/test_gpu_camera_branches.py): the same cases under the PERSPECTIVE CAMERA (view_type="point": csrc/ct_camera.hip, ct_camera_stack.hip,
ct_view_stack.hip).  A case carries `camera`, [3] or -- stack mode only -- [L,3], one position per shot, fp32-exact, in the point light's
coordinates; light_size is 1.0 for both light types (the camera's grid is the point light's).  `render` evaluates
tools/camera_oracle.cook_torrance_camera (image l of a per-shot stack: camera l and light l), `gradients` differentiates it and returns the
position's gradient as 'view', shaped like `camera`.  N.V, the half vector and N.H are read from the per-pixel view map F.normalize(C - P)
(of shot l), so they change sign from pixel to pixel; `decisions` lists n.v[l] per shot, and the angle grid skips angles against the
per-pixel dots.  Maps other than the normals (and `dark`'s solved albedo), lights, intensities and `view` are those of the build without a
camera.  `split_views`, per-shot mode only, puts three cameras on different sides of the surface under lights near +Z, so that the set of
shots that see the FRONT of the surface changes from pixel to pixel while all of them add into one pixel adjoint.
"""
import functools
import math
import os
import sys

import torch
import torch.nn.functional as TF

import blend_oracle as BO
import torch_oracle as O

MARGIN = 1e-3
BAND = 2e-5                     # the project's gradient band: |g - g64| <= BAND * (1 + |g64|)
KNEE_DECODE, KNEE_ENCODE = 0.04045, 0.0031308
ALBEDO_VALUES = (-0.2, 0.01, 0.03, 0.06, 0.5, 0.97, 1.3)

CASE_NAMES = ("backlit", "backview", "half_clamp", "saturated", "dark", "albedo_range", "closed_ends")
STACK_CASE_NAMES = CASE_NAMES + ("split_lights",)          # `split_lights` exists in stack mode only
VIEW_STACK_CASE_NAMES = STACK_CASE_NAMES + ("split_views",)    # `split_views` exists with one camera position per shot only

# name -> the variants of the case that the tests run (keyword arguments of `build`)
VARIANTS = {
    "backlit": [dict()],
    "backview": [dict()],
    "half_clamp": [dict()],
    "saturated": [dict()],
    "dark": [dict(return_srgb=True), dict(return_srgb=False)],
    # linear output: a channel whose albedo decodes to ~0 is dim, and the encode knee (which `dark` owns) would leave it undecided
    "albedo_range": [dict(return_srgb=False, **kw) for kw in (
        dict(workflow="metallic", albedo_is_srgb=True), dict(workflow="metallic", albedo_is_srgb=False),
        dict(workflow="specular", albedo_is_srgb=True), dict(workflow="specular", albedo_is_srgb=False),
        dict(workflow="converted", quirk=True, albedo_is_srgb=True), dict(workflow="converted", quirk=False, albedo_is_srgb=True),
        dict(workflow="converted", quirk=True, albedo_is_srgb=False))],
    "closed_ends": [dict()],
    "split_lights": [dict(return_srgb=True), dict(return_srgb=False)],
    "split_views": [dict(return_srgb=True), dict(return_srgb=False)],
}


# (h, w, light type, lights, tile) of every entry point of the chain rule that the GPU gradient tests are to drive; the host test
# holds every case to its caps at every one of them
ENTRY_CONFIGS = {
    "fp32-vector-lanes": (24, 40, "directional", 1, 1),
    "fp32-vector-lanes-point": (24, 40, "point", 1, 1),
    "fp32-one-pixel": (23, 37, "point", 1, 1),
    "multi-point": (24, 40, "point", 3, 1),
    "multi-directional": (24, 40, "directional", 3, 1),
    # the 16 x 120 one-tile launch is `crop(case, 120)` of this case, not a case built at 120 columns: under a directional light a pixel
    # shades the same wherever it is, so the two launches can be compared bit for bit on the shared columns
    "fp16-streamed": (16, 128, "directional", 1, 1),
    "fp16-streamed-point": (16, 128, "point", 1, 1),
    "tiled-sum-first": (12, 16, "directional", 1, 2),
    "tiled-point": (12, 16, "point", 1, 2),
    "tiled-two-kernels": (12, 18, "point", 1, 2),
}


# Stack mode: (h, w, light type, lights, fp16 maps) of every entry point of the LIGHT STACK (csrc/ct_stack.hip) -- the smallest shapes at
# which the angle grid still fills every branch of every case to 10 %
STACK_ENTRY_CONFIGS = {
    "stack-pairs": (24, 40, "directional", 3, False),         # two pixels per lane in the step, four-pixel lanes in the forward
    "stack-pairs-point": (24, 40, "point", 3, False),         # the x grid and row position per light
    "stack-one-pixel": (23, 37, "point", 3, False),           # odd width: one pixel per lane in the step, the forward's overlapping last lane
    "stack-fp16": (16, 64, "directional", 3, True),           # the __half instantiations
    "stack-fp16-point": (16, 64, "point", 3, True),
}


# Camera mode: (h, w, light type, lights, fp16 maps, mode) of every entry point of the perspective camera -- "sum": cook_torrance and the
# loss step with view_type="point" (csrc/ct_camera.hip); "camera_stack": the light stack under one camera position (csrc/ct_camera_stack.hip);
# "view_stack": one camera position per shot (csrc/ct_view_stack.hip).  The smallest shapes at which the angle grid still fills every branch
CAMERA_ENTRY_CONFIGS = {
    "camera-vector-lanes": (24, 40, "directional", 1, False, "sum"),           # forward 4-pixel lanes, backward pairs
    "camera-vector-lanes-point": (24, 40, "point", 1, False, "sum"),
    "camera-one-pixel": (23, 37, "point", 1, False, "sum"),                    # odd width: one pixel per lane
    "camera-multi-point": (24, 40, "point", 3, False, "sum"),                  # MULTI
    "camera-multi-directional": (24, 40, "directional", 3, False, "sum"),
    "camera-fp16": (16, 64, "directional", 1, True, "sum"),                    # the __half instantiations
    "camera-fp16-point": (16, 64, "point", 1, True, "sum"),
    "camera-stack-pairs-point": (24, 40, "point", 3, False, "camera_stack"),
    "camera-stack-one-pixel": (23, 37, "point", 3, False, "camera_stack"),     # and the forward stack's overlapping last lane
    "camera-stack-pairs": (24, 40, "directional", 3, False, "camera_stack"),
    "camera-stack-fp16": (16, 64, "point", 3, True, "camera_stack"),
    "view-stack-pairs-point": (24, 40, "point", 3, False, "view_stack"),
    "view-stack-one-pixel": (23, 37, "point", 3, False, "view_stack"),
    "view-stack-pairs": (24, 40, "directional", 3, False, "view_stack"),
    "view-stack-fp16": (16, 64, "directional", 3, True, "view_stack"),
}


def camera_entries(mode):
    return [e for e, c in CAMERA_ENTRY_CONFIGS.items() if c[5] == mode]


def build_for(entry, name, kw, seed=0):
    if entry in CAMERA_ENTRY_CONFIGS:
        h, w, light_type, n_lights, _, mode = CAMERA_ENTRY_CONFIGS[entry]
        return build(name, h, w, light_type=light_type, n_lights=n_lights, seed=seed, stack=mode != "sum",
                     camera="per_shot" if mode == "view_stack" else "fixed", **kw)
    if entry in STACK_ENTRY_CONFIGS:
        h, w, light_type, n_lights, _ = STACK_ENTRY_CONFIGS[entry]
        return build(name, h, w, light_type=light_type, n_lights=n_lights, seed=seed, stack=True, **kw)
    h, w, light_type, n_lights, tile = ENTRY_CONFIGS[entry]
    return build(name, h, w, light_type=light_type, n_lights=n_lights, tile=tile, seed=seed, **kw)


def stack_target(entry, name, kw, seed=0):
    """The MSE target of the stack tests for build_for(entry, name, kw, seed): the oracle's stack of ANOTHER material of the same case
    (seed ^ 1: other patterns, and the tilts mirrored, so a light behind the surface here is lit there and its target is not 0),
    [L,3,H,W] float32.  `dark`: lights 1 and 2 are behind every pixel of every seed, so their own images are 0 everywhere; light 1 takes
    light 0's image as its target instead, so that a light that must be masked has an upstream gradient that is not 0."""
    target = render(build_for(entry, name, kw, seed=seed ^ 1)).float()
    if name == "dark":
        target[1] = target[0]
    return target


def camera_target(entry, name, kw, seed=0):
    """The MSE target of the camera tests for build_for(entry, name, kw, seed), float32: the oracle's rendering of ANOTHER material of the
    same case (seed ^ 1), [3,H,W] for a "sum" entry, [L,3,H,W] for a stack entry (`dark`: as stack_target)."""
    target = render(build_for(entry, name, kw, seed=seed ^ 1)).float()
    if name == "dark" and target.dim() == 4:
        target[1] = target[0]
    return target


def crop(case, width):
    """The first `width` columns of an untiled case, maps and upstream weight alike."""
    assert case.tile == 1
    names = ("albedo", "normal", "roughness", "metallic", "specular")
    return case.replace(weight=case.weight[:, :, :width].contiguous(),
                        **{n: t[:, :, :width].contiguous() for n, t in zip(names, case.maps()) if t is not None})


def unfold(mask, k):
    """Map-grid mask -> output-grid mask (the inverse direction of a tiled map's repeats)."""
    return mask if k == 1 else mask.repeat(k, k)


def variant_id(name, kw):
    return name + "".join("-%s=%s" % (k, v) for k, v in sorted(kw.items()))


def all_variants():
    return [(n, kw) for n in CASE_NAMES for kw in VARIANTS[n]]


def all_stack_variants():
    return [(n, kw) for n in STACK_CASE_NAMES for kw in VARIANTS[n]]


def all_view_stack_variants():
    return [(n, kw) for n in VIEW_STACK_CASE_NAMES for kw in VARIANTS[n]]


def camera_variants(entry):
    """The variants a camera entry runs: the summed-lights ones, the stack ones, and with one camera per shot `split_views` too."""
    return {"sum": all_variants, "camera_stack": all_stack_variants, "view_stack": all_view_stack_variants}[CAMERA_ENTRY_CONFIGS[entry][5]]()


def _h(t):
    """Round to fp16-exact values."""
    return t.to(torch.float16).to(torch.float64)


class Case:
    """One set of inputs.  Maps are float64 tensors holding fp16-exact values: albedo [3,h,w], normal [3,h,w], roughness [1,h,w],
    metallic [1,h,w] | specular [3,h,w]; view [3]; lights, intensities [L,3]; weight [3,H,W] with (H, W) = tile * (h, w).
    `stack`: the case is a LIGHT STACK -- L images, one per light, each with its own clamp and encode, instead of one image of the
    summed lights; weight is then [L,3,H,W]."""

    camera = None          # camera mode: [3] one position, or [L,3] one per shot (stack mode only); fp32-exact

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def per_shot(self):
        return self.camera is not None and self.camera.dim() == 2

    @property
    def n_lights(self):
        return self.lights.shape[0]

    @property
    def out_shape(self):
        return (self.albedo.shape[1] * self.tile, self.albedo.shape[2] * self.tile)

    def maps(self):
        return (self.albedo, self.normal, self.roughness, self.metallic, self.specular)

    def map_names(self):
        return [n for n, t in zip(("albedo", "normal", "roughness", "metallic", "specular"), self.maps()) if t is not None]

    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        d.pop("_cache", None)
        return type(self)(**d)

    def product_kwargs(self):
        """Keyword arguments of pypbr_amd.functional.cook_torrance for this case (view / light tensors are added by the caller)."""
        kw = dict(light_type=self.light_type, light_size=self.light_size, albedo_is_srgb=self.albedo_is_srgb, return_srgb=self.return_srgb)
        if self.workflow == "converted":
            kw.update(convert_to_diffuse_specular=True, specular_is_srgb=self.quirk)
        elif self.workflow == "specular":
            kw.update(specular_is_srgb=self.specular_is_srgb)
        if self.tile != 1:
            kw.update(tile=self.tile)
        if self.camera is not None:
            kw.update(view_type="point")
        return kw


# ------------------------------------------------------------------------------------------------ the oracle on a case
def _rep(t, k):
    return t if (t is None or k == 1) else t.repeat(1, k, k)


def _render_inputs(case, maps, view, lights, intens):
    """-> (albedo, normal, roughness, metallic, specular, kwargs) of torch_oracle.cook_torrance[_multi] on the (repeated) maps;
    the converted workflow is metallic.py's conversion followed by the specular workflow, as torch_oracle.cook_torrance_converted."""
    a, n, r, m, s = [_rep(t, case.tile) for t in maps]
    kw = dict(view=view, light_type=case.light_type, light_size=case.light_size)
    if case.workflow == "converted":
        lin = O.srgb_to_linear(a) if case.albedo_is_srgb else a
        a, s = O.metallic_to_diffuse_specular(lin, m)
        m = None
        kw.update(albedo_is_srgb=False, specular_is_srgb=case.quirk)
    else:
        kw.update(albedo_is_srgb=case.albedo_is_srgb, specular_is_srgb=case.specular_is_srgb)
    return a, n, r, m, s, kw


def _camera_oracle():
    """tools/camera_oracle.py, the statement of view_type="point" that tests/test_camera_host.py pins to upstream pixel by pixel."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import camera_oracle
    return camera_oracle


def view_maps(case, camera=None, dtype=torch.float64):
    """-> list of L unit view maps [3,H,W] on the output grid, the one of shot l for light l: the expanded view direction, or in camera
    mode F.normalize(C - P) over the point light's grid (one map for every light, or with one camera per shot the map of camera l)."""
    H, W = case.out_shape
    L = case.n_lights
    if case.camera is None:
        v = TF.normalize(case.view.to(dtype), dim=0).view(3, 1, 1).expand(3, H, W)
        return [v] * L
    CO = _camera_oracle()
    cam = (case.camera if camera is None else camera).to(dtype)
    rows = cam.reshape(-1, 3)
    maps = [TF.normalize(CO.view_offsets(c, H, W, case.light_size), dim=0) for c in rows]
    return maps if len(maps) == L else maps * L


def _camera_render(case, maps, camera, lights, intens, dtype, view_map):
    CO = _camera_oracle()
    a, n, r, m, s, kw = _render_inputs(case, maps, None, lights, intens)
    common = dict(light_type=case.light_type, light_size=case.light_size, albedo_is_srgb=kw["albedo_is_srgb"],
                  specular_is_srgb=kw["specular_is_srgb"], return_srgb=case.return_srgb, dtype=dtype)
    if not case.stack:
        return CO.cook_torrance_camera(a, n, r, m, s, camera=camera, lights=lights, intensities=intens, view_map=view_map, **common)
    cams = camera.reshape(-1, 3)          # image l: camera l (or the one camera) and light l alone
    return torch.stack([CO.cook_torrance_camera(a, n, r, m, s, camera=cams[l if cams.shape[0] > 1 else 0], lights=lights[l:l + 1],
                                                intensities=intens[l:l + 1], view_map=view_map, **common) for l in range(lights.shape[0])])


def render(case, maps=None, view=None, lights=None, intens=None, dtype=torch.float64, view_map=None):
    """The oracle's rendering of the case (of other maps / parameters when given), in `dtype`.  Camera mode: `view` is the camera position(s),
    and `view_map` [3,H,W] forces one map of unit view vectors on every image instead."""
    maps = [None if t is None else t.to(dtype) for t in (case.maps() if maps is None else maps)]
    if case.camera is not None:
        return _camera_render(case, maps, (case.camera if view is None else view).to(dtype), (case.lights if lights is None else lights).to(dtype),
                              (case.intensities if intens is None else intens).to(dtype), dtype, view_map)
    view = (case.view if view is None else view).to(dtype)
    lights = (case.lights if lights is None else lights).to(dtype)
    intens = (case.intensities if intens is None else intens).to(dtype)
    a, n, r, m, s, kw = _render_inputs(case, maps, view, lights, intens)
    if case.stack:          # [L,3,H,W]: image l is the one-light evaluation for light l alone
        return torch.stack([O.cook_torrance(a, n, r, m, s, light=lights[l], intensity=intens[l], return_srgb=case.return_srgb, **kw)
                            for l in range(lights.shape[0])])
    if lights.shape[0] == 1:
        return O.cook_torrance(a, n, r, m, s, light=lights[0], intensity=intens[0], return_srgb=case.return_srgb, **kw)
    return O.cook_torrance_multi(a, n, r, m, s, lights=lights, intensities=intens, return_srgb=case.return_srgb, **kw)


def gradients(case, dtype=torch.float64, params=False, loss_target=None):
    """Autograd through the oracle of sum(out * weight) -- or of mse_loss(out, loss_target) -- in `dtype`.
    -> dict: map name -> gradient (map-sized: a tiled map owns the sum over its repeats), 'out' -> the rendering, and with
    params=True also 'view', 'lights', 'intensities' (camera mode: 'view' is the gradient of the camera position(s), shaped like them).
    A blend case: see _blend_gradients."""
    if getattr(case, "blend", False):
        assert not params and loss_target is None
        return _blend_gradients(case, dtype)
    leaves = [None if t is None else t.to(dtype).clone().requires_grad_(True) for t in case.maps()]
    P = [t.to(dtype).clone().requires_grad_(params) for t in (case.view if case.camera is None else case.camera, case.lights, case.intensities)]
    out = render(case, leaves, P[0], P[1], P[2], dtype)
    if loss_target is None:
        (out * case.weight.to(dtype)).sum().backward()
    else:
        TF.mse_loss(out, loss_target.to(dtype)).backward()
    res = {name: t.grad for name, t in zip(("albedo", "normal", "roughness", "metallic", "specular"), leaves) if t is not None}
    res["out"] = out.detach()
    if params:
        res.update(view=P[0].grad, lights=P[1].grad, intensities=P[2].grad)
    return res


def _terms(case, maps=None):
    """The reference's intermediate quantities in float64, from torch_oracle's own pieces (cooktorrance.py:92-182).
    -> dict with ndv [1,H,W] (ndv_l: per light, the N.V of its shot); per light lists ndl, ndh [1,H,W] and u [3,H,W] (the contribution
    BEFORE its clamp); base, f0.  Camera mode: N.V, the half vector and N.H come from the per-pixel view map (of shot l)."""
    dt = torch.float64
    maps = [None if t is None else t.to(dt) for t in (case.maps() if maps is None else maps)]
    a, n, r, m, s, kw = _render_inputs(case, maps, case.view, case.lights, case.intensities)
    base = O.srgb_to_linear(a) if kw["albedo_is_srgb"] else a
    if m is not None:
        f0 = torch.lerp(torch.full_like(base, 0.04), base, m)
    else:
        f0 = O.srgb_to_linear(s) if kw["specular_is_srgb"] else s
    _, H, W = base.shape
    vmaps = view_maps(case)                # per light: the view map of its shot (one and the same unless there is a camera per shot)
    nn = TF.normalize(n, dim=0)
    ndv_raws = [(nn * vmap).sum(dim=0, keepdim=True) for vmap in vmaps]
    res = dict(ndv=ndv_raws[0], ndv_l=ndv_raws, ndl=[], ndh=[], u=[], base=base, f0=f0, shade=[], rad=[])
    for l in range(case.n_lights):
        vmap, ndv = vmaps[l], ndv_raws[l].clamp(0, 1)
        lmap, att = O._light_geometry(case.light_type, case.lights[l].to(dt), case.light_size, H, W, dt, 0, H)
        half = TF.normalize(vmap + lmap, dim=0)
        cos_theta = torch.clamp((half * vmap).sum(dim=0, keepdim=True), 0.0, 1.0)
        fr = O._fresnel(cos_theta, f0)
        ndl_raw = (nn * lmap).sum(dim=0, keepdim=True)
        ndl = ndl_raw.clamp(0, 1)
        spec = (fr * O._ggx(nn, half, r) * O._smith(nn, vmap, lmap, r)) / (4.0 * ndv * ndl + 1e-7)
        kd = (1.0 - fr) * (1.0 - m) if m is not None else 1.0 - fr
        rad = case.intensities[l].to(dt).view(3, 1, 1) * (ndl * att)
        res["ndl"].append(ndl_raw)
        res["ndh"].append((nn * half).sum(dim=0, keepdim=True))
        res["u"].append((kd * base / math.pi + spec) * rad)
        res["shade"].append((kd / math.pi, spec))         # u = (shade[0] * base + shade[1]) * rad
        res["rad"].append(rad)
    return res


def decisions(case, maps=None):
    """-> list of (name, value [C,H,W] float64 on the OUTPUT grid, threshold, applies [C,H,W] bool | None, exact_ok)."""
    t = _terms(case, maps)
    maps = case.maps() if maps is None else maps
    k = case.tile
    if case.per_shot:
        out = [("n.v[%d]" % l, x, 0.0, None, False) for l, x in enumerate(t["ndv_l"])]
    else:
        out = [("n.v", t["ndv"], 0.0, None, False)]
    for l in range(case.n_lights):
        lit = t["ndl"][l] > -MARGIN          # skipped only where N.L is DECIDED negative (<= -MARGIN): the contribution is then 0 in any precision
        out.append(("n.l[%d]" % l, t["ndl"][l], 0.0, None, False))
        out.append(("n.h[%d]" % l, t["ndh"][l], 0.0, None, False))
        out.append(("u[%d] vs 0" % l, t["u"][l], 0.0, lit.expand_as(t["u"][l]), False))
        out.append(("u[%d] vs 1" % l, t["u"][l], 1.0, None, False))
    decoded = []
    if case.albedo_is_srgb:
        decoded.append(("albedo", _rep(maps[0].double(), k)))
    if case.workflow == "specular" and case.specular_is_srgb:
        decoded.append(("specular", _rep(maps[4].double(), k)))
    if case.workflow == "converted" and case.quirk:      # the converted specular map is decoded once more
        a = _rep(maps[0].double(), k)
        lin = O.srgb_to_linear(a) if case.albedo_is_srgb else a
        decoded.append(("converted specular", O.metallic_to_diffuse_specular(lin, _rep(maps[3].double(), k))[1]))
    for name, x in decoded:
        for thr in (0.0, KNEE_DECODE, 1.0):
            out.append(("%s vs %g" % (name, thr), x, thr, None, thr != KNEE_DECODE and case.name == "closed_ends"))
    if case.stack:          # every image is clamped and encoded by itself: no summed colour, one knee per light
        if case.return_srgb:      # a light decided behind has colour exactly 0 in any precision, more than MARGIN under the knee
            out += [("colour[%d] vs knee" % l, t["u"][l].clamp(0, 1), KNEE_ENCODE, None, False) for l in range(case.n_lights)]
        return out
    colour = t["u"][0].clamp(0, 1)
    if case.n_lights > 1:
        total = sum(u.clamp(0, 1) for u in t["u"])
        out.append(("sum vs 1", total, 1.0, None, False))
        colour = total.clamp(0, 1)
    if case.return_srgb:
        out.append(("colour vs knee", colour, KNEE_ENCODE, None, False))
    return out


def threshold_decided(case, maps=None):
    """[H,W] bool on the output grid: every compared quantity is at least MARGIN from its threshold."""
    ok = None
    for _, x, thr, applies, exact_ok in decisions(case, maps):
        good = (x - thr).abs() >= MARGIN
        if exact_ok:
            good = good | (x == thr)
        if applies is not None:
            good = good | ~applies
        good = good.all(dim=0)
        ok = good if ok is None else ok & good
    return ok


def _fold_all(mask, k):
    """Output-grid mask -> map-grid mask: a texel counts when every one of its k x k repeats does."""
    if k == 1:
        return mask
    H, W = mask.shape
    return mask.reshape(k, H // k, k, W // k).all(dim=2).all(dim=0)


def _cached(fn):
    @functools.wraps(fn)
    def wrapper(case):
        cache = case.__dict__.setdefault("_cache", {})
        if fn.__name__ not in cache:
            cache[fn.__name__] = fn(case)
        return cache[fn.__name__]
    return wrapper


@_cached
def reference(case):
    """float64 gradients of the case (computed once per case object, shared, never modified)."""
    return gradients(case, torch.float64)


@_cached
def well_conditioned(case):
    """[h,w] bool on the MAP grid: the oracle's own float32 gradients lie within half the band of its float64 gradients,
    for every map and channel."""
    g64, g32 = reference(case), gradients(case, torch.float32)
    ok = None
    for name in case.map_names():
        good = ((g32[name].double() - g64[name]).abs() <= 0.5 * BAND * (1 + g64[name].abs())).all(dim=0)
        ok = good if ok is None else ok & good
    return ok


@_cached
def decided(case):
    """[h,w] bool on the MAP grid: threshold-decided at every repeat, and well conditioned.  A blend case: and not `degenerate`."""
    ok = _fold_all(threshold_decided(case), case.tile) & well_conditioned(case)
    return ok & ~case.degenerate if getattr(case, "blend", False) else ok


def backlit(case):
    """[h,w] bool on the map grid: every light is behind the surface at every repeat (N.L < 0): all map gradients are exactly 0."""
    t = _terms(case)
    m = None
    for x in t["ndl"]:
        m = (x[0] < 0) if m is None else m & (x[0] < 0)
    return _fold_all(m, case.tile)


def behind(case):
    """[L,H,W] bool on the output grid: light l is DECIDED behind the surface (N.L <= -MARGIN): its contribution, and in a stack its
    whole image, is exactly 0 in any precision."""
    return torch.stack([x[0] <= -MARGIN for x in _terms(case)["ndl"]])


def branches(case):
    """-> dict name -> [H,W] bool on the output grid; 'named' is the branch the case is for, 'complement' the other side,
    further entries are sub-branches that the case promises too.  Stack mode: `saturated` and `dark` read every light's OWN colour."""
    t = _terms(case)
    L = case.n_lights
    ndv, ndl, ndh, u = t["ndv"][0], [x[0] for x in t["ndl"]], [x[0] for x in t["ndh"]], t["u"]
    ndvs = [x[0] for x in t["ndv_l"]]
    name = case.name
    if name == "backlit":
        return dict(named=functools.reduce(torch.logical_and, [x < 0 for x in ndl]), complement=functools.reduce(torch.logical_or, [x > 0 for x in ndl]))
    if name == "backview":      # one camera per shot: some shot seen from behind / every shot from the front
        return dict(named=functools.reduce(torch.logical_or, [x < 0 for x in ndvs]), complement=functools.reduce(torch.logical_and, [x > 0 for x in ndvs]))
    if name == "split_views":
        n_front = sum((x > 0).long() for x in ndvs)
        res = dict(named=(n_front >= 1) & (n_front < L), complement=n_front == L, one_front=n_front == 1, two_front=n_front == 2)
        res.update({"from_behind_%d" % l: x < 0 for l, x in enumerate(ndvs)})
        return res
    if name == "half_clamp":
        # several lights: a pixel is on the branch as soon as ONE light has N.H < 0 < N.L (each light runs the GGX term by itself),
        # and on the complementary branch only if no light has, while some light is lit with N.H > 0
        named = functools.reduce(torch.logical_or, [(h < 0) & (l > 0) for h, l in zip(ndh, ndl)])
        return dict(named=named, complement=functools.reduce(torch.logical_or, [(h > 0) & (l > 0) for h, l in zip(ndh, ndl)]) & ~named)
    if name == "split_lights":
        n_lit = sum((x > 0).long() for x in ndl)
        res = dict(named=(n_lit >= 1) & (n_lit < L), complement=n_lit == L, one_lit=n_lit == 1, two_lit=n_lit == 2)
        res.update({"behind_%d" % l: x < 0 for l, x in enumerate(ndl)})
        return res
    if name == "saturated" and case.stack:
        # the lights of one pixel on different sides of the clamp at 1: some light's own colour exceeds 1 in a channel while
        # another light's stays below 1 in every channel
        over = [(x > 1).any(dim=0) for x in u]
        below = [(x < 1).all(dim=0) for x in u]
        any_over = functools.reduce(torch.logical_or, over)
        return dict(named=any_over & functools.reduce(torch.logical_or, below), complement=~any_over)
    if name == "dark" and case.stack:      # per light, over the lit lights only (a light behind renders exactly 0)
        lit = [x > 0 for x in ndl]
        under = [(((x.clamp(0, 1) > 0) & (x.clamp(0, 1) < KNEE_ENCODE)).any(dim=0)) & k for x, k in zip(u, lit)]
        above = [(x.clamp(0, 1) > KNEE_ENCODE).all(dim=0) | ~k for x, k in zip(u, lit)]
        return dict(named=functools.reduce(torch.logical_or, under),
                    complement=functools.reduce(torch.logical_and, above) & functools.reduce(torch.logical_or, lit))
    if name == "saturated":
        alone = functools.reduce(torch.logical_or, [(x > 1).any(dim=0) for x in u])
        some_not = functools.reduce(torch.logical_or, [((x < 1).any(dim=0)) for x in u])
        res = dict(named=alone & some_not, complement=~alone)
        if L > 1:
            total = sum(x.clamp(0, 1) for x in u)
            each_below = functools.reduce(torch.logical_and, [x < 1 for x in u])          # per channel
            only_sum = ((total > 1) & each_below).any(dim=0)
            res.update(named=alone | only_sum, complement=~(alone | (total > 1).any(dim=0)), alone=alone, only_in_sum=only_sum)
        return res
    if name == "dark":
        colour = sum(x.clamp(0, 1) for x in u).clamp(0, 1)
        under = (colour > 0) & (colour < KNEE_ENCODE)
        return dict(named=under.any(dim=0), complement=(colour > KNEE_ENCODE).all(dim=0))
    k = case.tile
    a = _rep(case.albedo, k)
    if name == "albedo_range":
        x = torch.cat([a, _rep(case.specular, k)], 0) if case.workflow == "specular" else a
        ordinary = (x > KNEE_DECODE) & (x < 1)
        return dict(named=(~ordinary).any(dim=0), complement=ordinary.all(dim=0), below_zero=(x < 0).any(dim=0),
                    under_knee=((x > 0) & (x < KNEE_DECODE)).any(dim=0), above_one=(x > 1).any(dim=0))
    if name == "closed_ends":
        m = _rep(case.metallic, k)[0]
        ends = ((a == 0) | (a == 1)).any(dim=0) | (m == 0) | (m == 1)
        return dict(named=ends, complement=~ends, albedo_zero=(a == 0).any(dim=0), albedo_one=(a == 1).any(dim=0),
                    metallic_zero=m == 0, metallic_one=m == 1)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ building blocks
def _pattern(values, C, h, w, seed, step=(1, 3, 5)):
    """[C,h,w] of values from a list, by position: a fixed interleave (no random draw), shifted by the seed.  Blocks of
    2 x 4 texels share a value, so that the lanes of a vector group meet equal and different values."""
    v = torch.tensor(values, dtype=torch.float64)
    y = torch.arange(h).view(1, h, 1) // 2
    x = torch.arange(w).view(1, 1, w) // 4
    c = torch.arange(C).view(C, 1, 1)
    idx = (y * step[0] + x * step[1] + c * step[2] + seed) % len(values)
    return _h(v[idx])


def _tilted_normals(h, w, max_x, max_y, case_geom, reverse, min_x=None, keep=None):
    """Unit normals tilted about both axes on a grid of angles (degrees): columns sweep the tilt towards +-x over
    [-max_x, max_x], rows the tilt towards +-y over [-max_y, max_y].  Where a raw dot product with the view, a light or a
    half vector would be within 0.02 of zero the angle is SKIPPED: the pixel moves on along the grid by 3 degrees until all
    are clear.  N.L is kept further from zero (|N.L| >= 0.15): a lit pixel at a grazing light is so dim that its colour sits within
    MARGIN of the contribution's clamp at 0 or of the encode knee.  fp16-exact.
    `min_x`: the columns sweep [min_x, max_x] instead; `keep(n) -> [h,w] bool`: angles whose normal it rejects are skipped too."""
    ax = torch.linspace(-max_x if min_x is None else min_x, max_x, w, dtype=torch.float64).view(1, w).expand(h, w).clone()
    ay = torch.linspace(-max_y, max_y, h, dtype=torch.float64).view(h, 1).expand(h, w).clone()
    if reverse:
        ax = -ax if min_x is None else ax.flip(1)

    def make(ax, ay):
        rx, ry = torch.deg2rad(ax), torch.deg2rad(ay)
        n = torch.stack([torch.sin(rx) * torch.cos(ry), torch.sin(ry), torch.cos(rx) * torch.cos(ry)], 0)
        return _h(n * 0.75)                           # stored un-normalised on purpose (F.normalize, :154); fp16-exact

    n = make(ax, ay)
    for step in range(1, 24):
        dots = case_geom(n).abs()
        floor = torch.full((dots.shape[0], 1, 1), 0.02, dtype=torch.float64)
        floor[1:getattr(case_geom, "light_rows", None):2] = 0.15      # rows 1, 3, 5 ...: N.L of each light
        near = (dots < floor).any(dim=0)
        if keep is not None:
            near = near | ~keep(n)
        if not bool(near.any()):
            break
        shift = 3.0 * ((step + 1) // 2) * (1 if step % 2 else -1)
        ax2 = torch.where(near, (ax + shift).clamp(-80, 80), ax)
        n = torch.where(near.unsqueeze(0), make(ax2, ay), n)
    return n


def _geom_dots(view, lights, light_type, light_size, tile, camera=None):
    """-> function(normal [3,h,w]) -> [1 + 2 L, H, W] raw N.V, N.L and N.H on the output grid.  `camera` [3] | [L,3]: the view is the
    per-pixel map of the camera (of camera l for light l, and the N.V of shots 1 .. L-1 follow as rows 1 + 2 L ...)."""
    L = lights.shape[0]

    def f(n):
        n = TF.normalize(_rep(n, tile), dim=0)
        _, H, W = n.shape
        if camera is None:
            vs = [TF.normalize(view, dim=0).view(3, 1, 1).expand(3, H, W)] * L
        else:
            CO = _camera_oracle()
            vs = [TF.normalize(CO.view_offsets(c, H, W, light_size), dim=0) for c in camera.reshape(-1, 3)]
            vs = vs if len(vs) == L else vs * L
        rows = [(n * vs[0]).sum(0)]
        for l in range(L):
            lmap, _ = O._light_geometry(light_type, lights[l], light_size, H, W, torch.float64, 0, H)
            rows.append((n * lmap).sum(0))
            rows.append((n * TF.normalize(vs[l] + lmap, dim=0)).sum(0))
        if camera is not None and camera.dim() == 2:
            rows += [(n * v).sum(0) for v in vs[1:]]
        d = torch.stack(rows, 0)
        if tile != 1:          # a texel must be clear at every repeat
            k = tile
            d = d.reshape(d.shape[0], k, H // k, k, W // k)
            worst = d.abs().amin(dim=(1, 3))
            return worst
        return d
    f.light_rows = 1 + 2 * L                              # what follows is N.V again (of the other shots), not N.L
    return f


_POINT_DISTANCE = 2.5


def _lights(dirs, intens, light_type, distance=_POINT_DISTANCE):
    """Directions and intensities as given for a directional light; a point light sits `distance` along the same
    direction, its intensity raised by the squared distance (attenuation :140), so both types light the map alike."""
    d = torch.tensor(dirs, dtype=torch.float64)
    i = torch.tensor(intens, dtype=torch.float64)
    if light_type == "point":
        return TF.normalize(d, dim=1) * distance, i * distance ** 2
    return d, i


def _weight(H, W, seed):
    """Upstream gradient of both signs, |w| in [0.25, 1]."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.rand(3, H, W, generator=g, dtype=torch.float64) * 0.75 + 0.25
    sign = torch.where(torch.rand(3, H, W, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float().double()


ROUGHNESS_VALUES = (0.4, 0.55, 0.7, 0.85)


# What two cases are lit with in stack mode ONLY (directions, view and maps are the summed-lights case's; every other case keeps its
# intensities too).  Each image of a stack has its own clamp at 1:
#   saturated    the summed-lights intensities saturate all three lights in the same pixels; here light 0 saturates (red) where lights 1
#                and 2 stay below 1, so the lights of one pixel sit on different sides of the clamp
#   closed_ends  every image has its own encode knee; under the summed-lights intensities a channel with albedo 0 is so dim under the two
#                weaker lights that its colour is within MARGIN of the knee on 4.6-7.3 % of the pixels, over the 5 % cap: all three lights
#                are brighter here (0.1-0.5 % undecided)
STACK_INTENSITIES = {
    "saturated": [[9.0, 1.2, 2.4], [2.0, 0.6, 0.5], [2.0, 0.5, 0.6]],
    "closed_ends": [[4.5, 3.75, 5.25], [4.0, 4.5, 3.5], [3.5, 4.0, 4.5]],
}


# Camera mode: the camera sits CAMERA_DISTANCE along the case's own view direction (the map spans [-0.5, 0.5]^2, so the view direction
# changes by up to +-25 degrees across it); with one camera per shot, shot l is moved by CAMERA_DELTAS[l] (a handheld capture).
CAMERA_DISTANCE = 1.5
CAMERA_DELTAS = [[0.0, 0.0, 0.0], [0.15, -0.10, 0.05], [-0.20, 0.12, -0.04]]
# `half_clamp` (N.H < 0 < N.L lives at the steepest tilts towards +x, seen at a grazing angle from -x): under a point light the branch holds
# 6.0-6.5 % with the camera at 1.5 along the case's view, 9 % at 3.0, 0.1 % at 0.6.  Its camera is lower and further away (name -> direction,
# distance) and the columns sweep [-40, 80] degrees instead of [-80, 80] (name -> min_x, max_x): 12.5 % at the worst entry and seed.
CAMERA_PLACES = {"half_clamp": ([-0.995, 0.0, 0.1], 3.0)}
CAMERA_TILTS = {"half_clamp": (-40.0, 80.0)}
# `split_views`: low cameras on three sides.  The tilt grid runs with the pixel position, so perspective adds to the tilt at one seed and takes
# from it at the mirrored one; at elevation 0.5 the mirrored seed keeps one_front at 4 %, at 0.2 every (sub-)branch holds 19 % at both seeds.
SPLIT_VIEW_CAMERAS = [[0.8, 0.1, 0.2], [-0.8, 0.1, 0.2], [0.1, 0.8, 0.2]]
SPLIT_VIEW_TILTS = (75.0, 60.0)


def build(name, h, w, *, light_type="directional", n_lights=1, tile=1, seed=0, workflow="metallic", albedo_is_srgb=True,
          return_srgb=True, quirk=True, stack=False, flat=False, camera=None):
    """The case `name` on an h x w map (output tile*h x tile*w), one or three lights of one type.  stack=True: the same inputs read as a
    light stack (untiled); `split_lights` exists only so.  flat=True (build_blend only): every normal is one that a [0,1]-ENCODED map
    with three positive components decodes to (_flat_reachable); `backlit` is then lit and seen from the mirrored side.
    camera="fixed": CAMERA MODE, one camera position; camera="per_shot" (stack only): one position per light; `split_views` exists only so."""
    assert name in VIEW_STACK_CASE_NAMES and n_lights in (1, 3)
    assert not flat or (name != "half_clamp" and not stack)
    assert not stack or tile == 1
    assert name != "split_lights" or (stack and n_lights == 3)
    assert camera in (None, "fixed", "per_shot") and (camera is None or (tile == 1 and not flat))
    assert camera != "per_shot" or stack
    assert name != "split_views" or (camera == "per_shot" and n_lights == 3)
    specular_is_srgb = albedo_is_srgb
    # per case: view, light directions (the first is the case's own), intensities, tilt range, colours
    behind = [[0.1, -0.2, -1.0], [-0.3, 0.1, -0.9]]                      # lights under the surface: N.L < 0 at every tilt used with them
    albedo_values, metal_values = (0.4, 0.5, 0.7, 0.85), (0.0, 0.25, 0.5)
    max_x, max_y = 80.0, 80.0
    rough_values, point_distance = ROUGHNESS_VALUES, _POINT_DISTANCE
    if name == "backlit":
        view, dirs = [0.1, 0.05, 1.0], [[0.9, 0.25, 0.3], [0.8, 0.4, 0.25], [0.95, 0.1, 0.4]]
        intens = [[4.0, 3.5, 4.5]] * 3
        max_y = 50.0
    elif name == "backview":
        view, dirs = [-0.75, 0.15, 0.6], [[0.15, 0.2, 1.0], [0.3, -0.1, 0.9], [-0.1, 0.3, 0.95]]
        intens = [[4.0, 3.5, 4.5]] * 3
        max_y = 50.0
    elif name == "half_clamp":
        view, dirs = [-0.99, 0.0, 0.141], [[0.3, 0.0, 0.954], [0.35, 0.1, 0.93], [0.25, -0.1, 0.96]]
        intens = [[4.0, 3.5, 4.5]] * 3
        max_y = 40.0
    elif name == "split_lights":
        # three lights on different sides of the surface: which of them are lit changes from pixel to pixel
        view, dirs = [0.1, 0.05, 1.0], [[0.8, 0.1, 0.5], [-0.8, 0.1, 0.5], [0.1, 0.8, 0.5]]
        intens = [[4.0, 3.5, 4.5], [3.0, 4.0, 3.5], [3.5, 3.0, 4.0]]
        max_y = 60.0
    elif name == "split_views":
        # three cameras on different sides of the surface (SPLIT_VIEW_CAMERAS), every light near +Z: which shots see the front of the
        # surface changes from pixel to pixel, while almost every pixel is lit in every shot
        view, dirs = [0.1, 0.05, 1.0], [[0.15, 0.2, 1.0], [0.3, -0.1, 0.9], [-0.1, 0.3, 0.95]]
        intens = [[4.0, 3.5, 4.5], [3.0, 4.0, 3.5], [3.5, 3.0, 4.0]]
        max_x, max_y = SPLIT_VIEW_TILTS
    elif name == "saturated":
        view, dirs = [0.1, -0.1, 1.0], [[0.2, 0.1, 1.0], [-0.2, 0.2, 1.0], [0.1, -0.3, 1.0]]
        intens = [[9.0, 1.2, 2.4], [7.0, 0.6, 0.5], [7.0, 0.5, 0.6]]
        albedo_values, metal_values = (0.97, 0.5, 0.97, 0.25, 0.5), (0.0, 0.25)
        max_x = max_y = 35.0
    elif name == "dark":
        view, dirs = [0.1, -0.1, 1.0], [[0.2, 0.1, 1.0]] + behind
        intens = [[0.04, 0.04, 0.04]] * 3
        metal_values = (0.0,)
        max_x = max_y = 30.0
        rough_values = (0.55, 0.7, 0.85)
        point_distance = 4.0
    else:      # albedo_range, closed_ends: light and view near +Z and shallow tilts, so that a channel whose albedo decodes to ~0
        # still shows a specular term well above MARGIN and the encode knee
        view, dirs = [0.1, -0.1, 1.0], [[0.25, 0.15, 1.0], [-0.3, 0.2, 0.9], [0.1, -0.35, 1.0]]
        # the converted workflow with the double decode has f0 <= decode(0.04) = 0.003 where the albedo is ~0: it needs more light
        k = 10.0 if (workflow == "converted" and quirk) else 1.0
        intens = [[3.0 * k, 2.5 * k, 3.5 * k]] * 3 if n_lights == 1 else [[3.0 * k, 2.5 * k, 3.5 * k], [2.4 * k, 2.0 * k, 2.6 * k], [2.0 * k, 2.2 * k, 1.8 * k]]
        max_x = max_y = 25.0
        rough_values = (0.55, 0.7, 0.85)
    if name == "saturated" and n_lights == 1:
        intens = [[9.0, 1.2, 2.4]]
    min_x = None
    if flat and name in ("backlit", "backview"):
        # tilts towards -x beyond about 50 degrees have no encoding with three positive components: the columns sweep [-35, 80] and the
        # rows +-35; `backlit`'s lights (and view) are mirrored in x, so that the lights are behind at the tilts towards +x
        min_x, max_y = -35.0, 35.0
        if name == "backlit":
            view, dirs = [-view[0], view[1], view[2]], [[-d[0], d[1], d[2]] for d in dirs]
    if stack and name in STACK_INTENSITIES:
        intens = STACK_INTENSITIES[name]
    lights, intensities = _lights(dirs[:n_lights], intens[:n_lights], light_type, point_distance)
    lights, intensities = lights.float().double(), intensities.float().double()          # fp32-exact: the kernels take them as floats
    view = torch.tensor(view, dtype=torch.float32).double()
    light_size = 1.0 if light_type == "point" else None
    cam = None
    if camera is not None:
        light_size = 1.0                                  # the camera's grid is the point light's, for both light types
        direction, distance = CAMERA_PLACES.get(name, (view.tolist(), CAMERA_DISTANCE))
        cam = TF.normalize(torch.tensor(direction, dtype=torch.float64), dim=0) * distance
        if camera == "per_shot":
            cam = cam.view(1, 3) + torch.tensor(CAMERA_DELTAS[:n_lights], dtype=torch.float64)
            if name == "split_views":
                cam = TF.normalize(torch.tensor(SPLIT_VIEW_CAMERAS, dtype=torch.float64), dim=1) * CAMERA_DISTANCE
        cam = cam.float().double()                        # fp32-exact: the kernels take it as floats
        if name in CAMERA_TILTS:
            min_x, max_x = CAMERA_TILTS[name]
    # half_clamp's branch lives at the steepest tilts towards +x: they come FIRST, so that cutting a map's last columns keeps them
    reverse = (seed % 2 == 1) != (name == "half_clamp")
    normal = _tilted_normals(h, w, max_x, max_y, _geom_dots(view, lights, light_type, light_size, tile, camera=cam), reverse,
                             min_x=min_x, keep=_flat_reachable if flat else None)
    rough = _pattern(rough_values, 1, h, w, seed + 1, step=(3, 1, 0))
    albedo = _pattern(albedo_values, 3, h, w, seed)
    metallic = _pattern(metal_values, 1, h, w, seed + 2, step=(1, 2, 0)) if workflow != "specular" else None
    specular = _pattern((0.3, 0.5, 0.97, 0.7), 3, h, w, seed + 3, step=(2, 1, 3)) if workflow == "specular" else None
    if name in ("albedo_range", "closed_ends"):
        # texel classes in 2 x 4 blocks: 0 = every channel ordinary (the complementary branch), 1 and 2 = the listed values
        cls = _pattern((0.0, 1.0, 2.0, 1.0), 1, h, w, seed + 4, step=(1, 1, 0))
        if name == "albedo_range":
            ordinary = _pattern((0.06, 0.5, 0.97, 0.3), 3, h, w, seed + 5)
            listed = _pattern(ALBEDO_VALUES, 3, h, w, seed)
            albedo = torch.where(cls == 0, ordinary, listed)
            if workflow == "specular":
                # class 2: the SPECULAR map takes the listed values under an ordinary albedo (both ~0 in one channel would render ~0 there)
                albedo = torch.where(cls == 2, _pattern((0.5, 0.97, 0.7), 3, h, w, seed + 6), albedo)
                specular = torch.where(cls == 2, _pattern(ALBEDO_VALUES, 3, h, w, seed + 1, step=(1, 2, 3)), specular)
            elif workflow == "converted":
                metallic = _pattern((0.5, 0.75), 1, h, w, seed + 2, step=(1, 2, 0))
            else:
                metallic = _pattern((0.0, 0.25, 0.5, 0.75), 1, h, w, seed + 2, step=(1, 2, 0))
        else:
            ends_a = _pattern((0.0, 1.0, 0.5, 1.0, 0.25, 0.0, 0.75), 3, h, w, seed)
            ends_m = _pattern((0.0, 1.0, 0.5, 0.0, 0.25), 1, h, w, seed + 2, step=(1, 2, 0))
            albedo = torch.where(cls == 0, _pattern((0.5, 0.25, 0.75), 3, h, w, seed + 5), ends_a)
            metallic = torch.where(cls == 0, _pattern((0.25, 0.5), 1, h, w, seed + 6), ends_m)
            # a black metal (albedo 0, metallic 1) renders ~0 in that channel, which is within MARGIN of the contribution's clamp
            # at 0: metallic 1 goes with albedo 1 / interior values, metallic 0 with every albedo
            albedo = torch.where((metallic == 1.0) & (albedo == 0.0), torch.ones_like(albedo), albedo)
    H, W = h * tile, w * tile
    case = Case(name=name, albedo=albedo, normal=normal, roughness=rough, metallic=metallic, specular=specular, view=view, lights=lights,
                intensities=intensities, light_type=light_type, light_size=light_size, workflow=workflow, albedo_is_srgb=albedo_is_srgb,
                specular_is_srgb=specular_is_srgb, return_srgb=return_srgb, quirk=quirk, tile=tile, stack=stack, camera=cam,
                weight=_weight(H, W, 1000 + seed) if not stack else torch.stack([_weight(H, W, 1000 + seed + 100 * l) for l in range(n_lights)]))
    if name == "dark":
        case = _solve_dark(case, seed)
    return case


DARK_TARGETS = (1.4e-3, 1.5e-3, 1.6e-3)          # linear colours inside (MARGIN, knee - MARGIN)
LIT_TARGETS = (5.2e-3, 5.6e-3, 6.0e-3)           # ... and above knee + MARGIN: the complementary branch


def _solve_dark(case, seed):
    """`dark`: the albedo of every texel is SOLVED for, so that the linear colour of each channel is one of DARK_TARGETS (half of
    the 2 x 4 blocks) or of LIT_TARGETS (the others).  With metallic = 0 the contribution is (kd base / pi + spec) rad (:169-176),
    linear in base.  Tiled maps: solved for the mean over the repeats (a point light shades them a little differently)."""
    h, w = case.albedo.shape[1:]
    k = case.tile
    trial = case.replace(albedo=torch.full_like(case.albedo, 0.5), albedo_is_srgb=False)
    t = _terms(trial)
    fold = lambda x: x.reshape(x.shape[0], k, h, k, w).mean(dim=(1, 3))
    kd_pi, spec = t["shade"][0]
    slope, offset = fold(kd_pi * t["rad"][0]), fold(spec * t["rad"][0])
    dark = _pattern((1.0, 0.0), 1, h, w, seed, step=(1, 1, 0)) == 1.0
    target = torch.where(dark, _pattern(DARK_TARGETS, 3, h, w, seed, step=(1, 1, 1)), _pattern(LIT_TARGETS, 3, h, w, seed, step=(1, 1, 1)))
    base = (target - offset) / slope
    if case.albedo_is_srgb:      # store the sRGB encoding (functions.py:50-66 inverted)
        base = torch.where(base <= KNEE_ENCODE, base * 12.92, 1.055 * base.clamp_min(1e-9) ** (1 / 2.4) - 0.055)
    return case.replace(albedo=_h(base))


def fill_undecided(case):
    """For gradients that are sums over all pixels (view, light, intensity): texels that are not decided take the values of a
    decided neighbour -- tried in a fixed order of offsets, and taken only when they are decided at the new place too.
    -> (case, share of texels still undecided)."""
    cur = case
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0), (0, 4), (0, -4), (2, 0), (-2, 0), (2, 4), (-2, -4), (0, 8), (4, 0)):
        bad = ~decided(cur)
        if not bool(bad.any()):
            break
        maps = [None if t is None else torch.where(bad.unsqueeze(0), torch.roll(t, (dy, dx), (1, 2)), t) for t in cur.maps()]
        trial = cur.replace(**dict(zip(("albedo", "normal", "roughness", "metallic", "specular"), maps)))
        take = bad & decided(trial)
        maps = [None if t is None else torch.where(take.unsqueeze(0), n, t) for t, n in zip(cur.maps(), maps)]
        cur = cur.replace(**dict(zip(("albedo", "normal", "roughness", "metallic", "specular"), maps)))
    return cur, float((~decided(cur)).double().mean())


def report(case):
    """One line: branch populations and undecided share (what the host test prints)."""
    b = branches(case)
    d = decided(case)
    parts = ["%s %.1f%%" % (k, 100 * float(v.double().mean())) for k, v in b.items()]
    return "%-13s %dx%d tile %d %-11s L=%d %-9s | %s | undecided %.2f%% (thresholds %.2f%%, conditioning %.2f%%)" % (
        case.name, case.albedo.shape[1], case.albedo.shape[2], case.tile, case.light_type, case.n_lights, case.workflow, ", ".join(parts),
        100 * float((~d).double().mean()), 100 * float((~_fold_all(threshold_decided(case), case.tile)).double().mean()),
        100 * float((~well_conditioned(case)).double().mean()))


# ------------------------------------------------------------------------------------------------ blend mode
# BLEND MODE (build_blend, BLEND_ENTRY_CONFIGS; held by tests/test_blend_branches_host.py, run on the GPU by tests/test_gpu_blend_branches.py):
# two materials and a mask whose BLEND (blend_oracle.blend_materials: lerp of the plain maps, normalize / lerp / normalize of the normals, the
# blended normal decoded again when the whole map has no negative component) is the case `name`.  The case object carries the blended maps in
# float64 as its own maps, so `decisions`, `threshold_decided`, `branches` and `backlit` read the blend from the oracle alone; `gradients`
# differentiates sum(out * W) through the blend and the render for both materials' maps and the mask, `well_conditioned` compares all of them.
# Inputs are fp32-exact (the fused blend is fp32 only).
MAP_NAMES = ("albedo", "normal", "roughness", "metallic", "specular")
MASK_VALUES = (0.0, 0.25, 0.5, 0.75, 1.0, 0.5)
THETA_VALUES = (6.0, -9.0, 12.0, -5.0)            # degrees between the two materials' normals
DELTA_VALUES = (0.1, -0.15, 0.2, -0.05)           # material 1 - material 2 of a plain map (roughness: half of it)
STORED_LENGTHS = (0.75, 1.25)                     # the two normals are stored un-normalised, at different lengths

# (h, w, light type, lights, tile): the smallest shapes that still fill every branch to 10 %
BLEND_ENTRY_CONFIGS = {
    "blend-pairs": (24, 40, "directional", 1, 1),             # two pixels per lane
    "blend-pairs-point": (24, 40, "point", 1, 1),
    "blend-one-pixel": (23, 37, "point", 1, 1),               # odd width: one pixel per lane
    "blend-multi-point": (24, 40, "point", 3, 1),             # MULTI
    "blend-multi-directional": (24, 40, "directional", 3, 1),
    "blend-tiled": (12, 16, "directional", 1, 2),             # the fused tiled backward (ct_repeat_backward.hpp)
    "blend-tiled-point": (12, 16, "point", 1, 2),
    "blend-pieces": (24, 40, "point", 1, 1),                  # the unfused differentiable pieces, called directly
}


def all_blend_variants():
    """Every variant signed (the blended normal map has negative components: kept as it is), every case but `half_clamp` flat (every
    component positive everywhere: decoded again), and one dedicated variant with `degenerate` texels."""
    out = [(n, dict(kw)) for n, kw in all_variants()]
    out += [(n, dict(kw, flat=True)) for n, kw in all_variants() if n != "half_clamp"]
    out.append(("backview", dict(degenerate=True)))
    return out


class BlendCase(Case):
    """A Case whose maps are the float64 BLEND of `first` and `second` (dicts name -> [C,h,w] float64 of fp32-exact values) under `mask`
    [1,h,w]; `flat`: the blended normal map counts as [0,1]-encoded; `degenerate` [h,w] bool: texels kept out of every comparison."""
    blend = True

    def map_names(self):
        """The names of the gradients: '1.albedo' ... '2.metallic', 'mask'."""
        return ["%d.%s" % (i, n) for i, m in ((1, self.first), (2, self.second)) for n in MAP_NAMES if m.get(n) is not None] + ["mask"]


def _f(t):
    """Round to fp32-exact values."""
    return t.float().double()


def _flat_encode(nn):
    """Unit normals -> the unit vectors o with normalize(2 o - 1) = nn:  o = (1 + s nn) / 2,  s = -sigma + sqrt(sigma^2 + 1),
    sigma = nn_x + nn_y + nn_z  (|o| = 1 is a quadratic in s)."""
    sigma = nn.sum(dim=0, keepdim=True)
    return (1 + (-sigma + torch.sqrt(sigma * sigma + 1)) * nn) / 2


def _flat_reachable(n):
    """[h,w] bool: the encoding of this normal has three components of at least 0.05 (positive with room for the blend's own error)."""
    return (_flat_encode(TF.normalize(n, dim=0)) >= 0.05).all(dim=0)


def blended_maps(first, second, mask, dtype=torch.float64):
    """The oracle's blend of two materials, as the five maps of a Case."""
    bl = BO.blend_materials({k: v.to(dtype) for k, v in first.items()}, {k: v.to(dtype) for k, v in second.items()}, mask.to(dtype))
    return [bl.get(n) for n in MAP_NAMES]


def blend_is_flat(case):
    """The whole-map flag, from the oracle: no component of the blended normal map (before it is assigned) is negative or zero."""
    return bool(BO.blend_normals(case.first["normal"], case.second["normal"], case.mask).min() > 0)


DEGENERATE_BLOCKS = ((6, 8), (14, 24))            # (row, column) of two 2 x 4 blocks: opposed normals under mask 0.5; a stored (0, 0, 0)


def _split(x, seed, flat, degenerate):
    """x = w m1 + (1 - w) m2 for every plain map (m1 = x + (1 - w) d, m2 = x - w d), and for the normal a^ = cos((1-w) th) n + sin((1-w) th) t,
    b^ = cos(w th) n - sin(w th) t with t a tangent: the two unit normals th degrees apart, their blend along n.  flat: n is the ENCODING of the
    case's normal.  `closed_ends`: where x is exactly 0.0 or 1.0 both materials hold that value (d = 0), so the blend is that number in any precision."""
    h, w = x.albedo.shape[1:]
    mask = _pattern(MASK_VALUES, 1, h, w, 7 + seed, step=(1, 2, 0))
    deg = torch.zeros(h, w, dtype=torch.bool)
    if degenerate:
        assert 16 <= 0.02 * h * w, "the degenerate class is at most 2 % of the texels"
        for y0, x0 in DEGENERATE_BLOCKS:
            deg[y0:y0 + 2, x0:x0 + 4] = True
        y0, x0 = DEGENERATE_BLOCKS[0]
        mask[:, y0:y0 + 2, x0:x0 + 4] = 0.5
    first, second = {}, {}
    for i, (name, t) in enumerate(zip(MAP_NAMES, x.maps())):
        if t is None:
            continue
        if name == "normal":
            n = TF.normalize(t, dim=0)
            if flat:
                n = TF.normalize(_flat_encode(n), dim=0)
            axis = torch.tensor([0.3, 0.9, 0.2], dtype=torch.float64).view(3, 1, 1).expand_as(n)
            tang = TF.normalize(torch.cross(n, axis, dim=0), dim=0)
            th = torch.deg2rad(_pattern(THETA_VALUES, 1, h, w, seed + 9, step=(1, 1, 0)))
            a = n * torch.cos((1 - mask) * th) + tang * torch.sin((1 - mask) * th)
            b = n * torch.cos(mask * th) - tang * torch.sin(mask * th)
            first[name], second[name] = _f(a * STORED_LENGTHS[0]), _f(b * STORED_LENGTHS[1])
            if degenerate:
                (y0, x0), (y1, x1) = DEGENERATE_BLOCKS
                up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).view(3, 1, 1)
                first[name][:, y0:y0 + 2, x0:x0 + 4] = up * STORED_LENGTHS[0]          # exactly opposed: the blend has length 0
                second[name][:, y0:y0 + 2, x0:x0 + 4] = -up * STORED_LENGTHS[1]
                second[name][:, y1:y1 + 2, x1:x1 + 4] = 0.0
        else:
            d = _pattern(DELTA_VALUES, t.shape[0], h, w, seed + 11 + i) * (0.5 if name == "roughness" else 1.0)
            if x.name == "closed_ends":
                d = torch.where((t == 0) | (t == 1), torch.zeros_like(d), d)
            first[name], second[name] = _f(t + (1 - mask) * d), _f(t - mask * d)
    return first, second, mask, deg


def _first_for(x, shared, flat):
    """Material 1 whose blend with ANOTHER blend case's material 2 and mask is x (a batch of first materials against one second material):
    m1 = (x - (1 - w) m2) / w, and for the normal the unit a^ with w a^ + (1 - w) b^ along n.  Where the mask is 0 the blend is material 2."""
    w = shared.mask
    safe = torch.where(w > 0, w, torch.ones_like(w))
    first = {}
    for name, t in zip(MAP_NAMES, x.maps()):
        if t is None:
            continue
        m2 = shared.second[name]
        if name == "normal":
            n = TF.normalize(t, dim=0)
            if flat:
                n = TF.normalize(_flat_encode(n), dim=0)
            b = TF.normalize(m2, dim=0)
            c = (1 - w) * (n * b).sum(dim=0, keepdim=True)
            lam = c + torch.sqrt((c * c - (1 - w) ** 2 + w ** 2).clamp_min(0.0))          # |lam n - (1 - w) b^| = w
            first[name] = _f(torch.where(w > 0, (lam * n - (1 - w) * b) / safe, n))
        else:
            first[name] = _f(torch.where(w > 0, (t - (1 - w) * m2) / safe, t))
    return first


def build_blend(name, h, w, *, flat=False, degenerate=False, shared=None, seed=0, **kw):
    """Two materials and a mask whose blend is the case `name` (keyword arguments of `build`).  flat=True: every component of the blended
    normal map is positive, so it is decoded again.  shared=<blend case>: its material 2 and mask, and the material 1 that blends to this case."""
    x = build(name, h, w, seed=seed, flat=flat, **kw)
    if shared is None:
        first, second, mask, deg = _split(x, seed, flat, degenerate)
    else:
        first, second, mask, deg = _first_for(x, shared, flat), shared.second, shared.mask, shared.degenerate
    d = dict(x.__dict__)
    d.pop("_cache", None)
    d.update(zip(MAP_NAMES, blended_maps(first, second, mask)))
    return BlendCase(**dict(d, first=first, second=second, mask=mask, flat=flat, degenerate=deg))


def build_blend_for(entry, name, kw, seed=0, shared=None):
    h, w, light_type, n_lights, tile = BLEND_ENTRY_CONFIGS[entry]
    return build_blend(name, h, w, light_type=light_type, n_lights=n_lights, tile=tile, seed=seed, shared=shared, **kw)


def _blend_gradients(case, dtype):
    """Autograd of sum(out * weight) through blend_oracle.blend_materials and the render, in `dtype`.
    -> dict: '1.<map>' / '2.<map>' / 'mask' -> gradient (map-sized), 'out' -> the rendering."""
    r1 = {k: v.to(dtype).clone().requires_grad_(True) for k, v in case.first.items()}
    r2 = {k: v.to(dtype).clone().requires_grad_(True) for k, v in case.second.items()}
    rm = case.mask.to(dtype).clone().requires_grad_(True)
    bl = BO.blend_materials(r1, r2, rm)
    out = render(case, [bl.get(n) for n in MAP_NAMES], dtype=dtype)
    (out * case.weight.to(dtype)).sum().backward()
    res = {"%d.%s" % (i, k): v.grad for i, m in ((1, r1), (2, r2)) for k, v in m.items()}
    res.update(mask=rm.grad, out=out.detach())
    return res


# A batch of two first materials (seeds 0 and 2) against ONE second material and ONE mask (those of seed 0), one per light type
BLEND_BATCH_CASES = (("blend-pairs", "backlit", dict()), ("blend-pairs-point", "saturated", dict(flat=True)))


def build_blend_batch(entry, name, kw):
    first = build_blend_for(entry, name, kw, seed=0)
    return [first, build_blend_for(entry, name, kw, seed=2, shared=first)]
