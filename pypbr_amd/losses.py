"""`RenderingLoss`: the rendering loss of the reference's tutorial (docs/source/tutorials/06_advanced.rst:73-107) as a module.

Upstream the class lives in the tutorial, not in the package:

    rendered_pred = self.brdf(predicted_material, self.view_dir, self.light_dir, self.light_intensity)
    rendered_gt = self.brdf(ground_truth_material, self.view_dir, self.light_dir, self.light_intensity)
    loss = nn.MSELoss()(rendered_pred, rendered_gt)

Same constructor, same forward arguments, same value and gradients here.  The ground-truth rendering is one launch of the fused
evaluation; it runs without a graph when nothing it depends on requires grad (the usual case: the predicted material's evaluation,
the MSE and their backward are then ONE kernel, functional.rendering_loss_mse -> pbr_cook_torrance_mse_step, whenever the predicted
maps are plain tensors on a ROCm device).  When `view_dir` / `light_dir` / `light_intensity` -- shared by both renderings upstream --
or a ground-truth map require grad, the ground truth is rendered differentiably, as upstream renders it: a light being fitted receives
the gradient of BOTH branches.
"""
import torch
import torch.nn as nn

from . import functional as F_
from .models import CookTorranceBRDF


def _plain_maps(brdf, material):
    """(albedo, normal, roughness, metallic, specular) of a material as the one-pass entry points can read them in place -- specular None
    beside a metallic map -- else None: the material takes the composition through the BRDF module, which handles whatever it is handed
    (CPU-resident maps, a lazy blend, maps not yet decoded)."""
    a, n, r, m, s = material._stored(("albedo", "normal", "roughness", "metallic", "specular"))
    ok = (material._is_materialised(allow_tile=brdf.view_type != "point")      # the camera renders real maps: the module materialises
          and torch.device(material.device).type == "cuda"
          and a is not None and r is not None and material._stores("normal")
          and (m is not None or s is not None) and all(t is None or t.is_cuda for t in (a, n, r, m, s))
          and brdf.override_device is None)
    return (a, n, r, m, None if m is not None else s) if ok else None


def _reference(ground_truth, shared, render):
    """The reference of a loss: `ground_truth` itself when it is a tensor, else `render(ground_truth)`.  06_advanced.rst:101-102 renders
    both materials under autograd.  Without a graph only when nothing could receive a gradient through this branch: no ground-truth map
    and none of the `shared` light / view tensors requires grad."""
    if isinstance(ground_truth, torch.Tensor):
        return ground_truth
    differentiable = torch.is_grad_enabled() and any(
        isinstance(t, torch.Tensor) and t.requires_grad for t in ground_truth._render_inputs() + list(shared))
    with torch.enable_grad() if differentiable else torch.no_grad():
        return render(ground_truth)


class RenderingLoss(nn.Module):
    def __init__(self, light_type='point', view_dir=torch.tensor([0.0, 0.0, 1.0]), light_dir=torch.tensor([0.1, 0.1, 1.0]),
                 light_intensity=torch.tensor([1.0, 1.0, 1.0]), light_size=None, view_type='directional'):
        super().__init__()
        self.brdf = CookTorranceBRDF(light_type=light_type, view_type=view_type)    # 'point': `view_dir` is the camera's position (models.py)
        self.view_dir = view_dir
        self.light_dir = light_dir
        self.light_intensity = light_intensity
        self.light_size = light_size

    def _render(self, material):
        return self.brdf(material, self.view_dir, self.light_dir, self.light_intensity, self.light_size)

    def forward(self, predicted_material, ground_truth_material, weights=None):
        """`ground_truth_material`: a material, or the reference rendering itself ((3,H,W) / (B,3,H,W) tensor).  `weights` (an extension):
        one weight per pixel, (1,H,W) / (B,1,H,W); the loss is `(weights * (rendering - reference) ** 2).mean()`
        (functional.rendering_loss_mse(weights=))."""
        rendered_gt = _reference(ground_truth_material, (self.view_dir, self.light_dir, self.light_intensity), self._render)
        maps = _plain_maps(self.brdf, predicted_material)
        if maps is None:
            rendered_pred = self._render(predicted_material)
            if weights is not None:
                return F_._weighted_mse(rendered_pred, rendered_gt, weights)
            return nn.MSELoss()(rendered_pred, rendered_gt.to(rendered_pred.device))
        return F_.rendering_loss_mse(*maps, target=rendered_gt.to(maps[0].device), view_dir=self.view_dir, light=self.light_dir,
                                     light_intensity=self.light_intensity, light_type=self.brdf.light_type, light_size=self.light_size,
                                     view_type=self.brdf.view_type, **({} if weights is None else {"weights": weights}),
                                     tile=predicted_material.lazy_tile,      # a recorded tile(n): evaluated and differentiated at every repeat
                                     albedo_is_srgb=bool(predicted_material.albedo_is_srgb),
                                     specular_is_srgb=bool(getattr(predicted_material, "specular_is_srgb", True)))


class MultiLightRenderingLoss(nn.Module):
    """The same loss over a LIGHT STACK (an extension: upstream has only the tutorial's loss, applied here to L images): a capture of L
    photographs from one camera position with the light moved between the shots.  `lights` [L,3] (1 <= L <= 16, one light type),
    `light_intensities` [3] / [1,3] for all lights or [L,3], one `view_dir`, one `light_size`.  The loss is nn.MSELoss() over the L renderings
    of the predicted material against `ground_truth` -- a material, rendered with ONE launch (functional.cook_torrance_stack), or the stack
    of photographs itself ([L,3,H,W] / [B,L,3,H,W]).  When the ground truth is rendered differentiably, and when the predicted material takes
    the one-pass form (functional.rendering_loss_mse_stack -> pbr_cook_torrance_mse_stack_step), follows RenderingLoss's rules.
    With photographs as `ground_truth`, `lights`, `light_intensities` or `view_dir` that require grad -- plain tensors, or nn.Parameters,
    which nn.Module registers on assignment so that `loss.parameters()` yields them -- are fitted in the same pass
    (pbr_cook_torrance_mse_stack_fit_step); through a differentiably rendered ground truth they take the composition.  With
    view_type='point' (`view_dir` is the camera's position) the one launch and the two passes are the camera's own
    (pbr_cook_torrance_camera_stack, pbr_cook_torrance_camera_mse_stack_step, pbr_cook_torrance_camera_mse_stack_fit_step), under the same
    rules; the gradient `view_dir` receives is the position's.  `view_dir` [L,3] is one view per shot -- with view_type='point' a handheld
    capture, the camera moving with the flash -- and reaches functional's per-shot routes (pbr_cook_torrance_view_stack,
    pbr_cook_torrance_view_mse_stack_step, pbr_cook_torrance_view_mse_stack_fit_step); its gradient comes back [L,3].
    `forward(..., weights=)` takes one weight per pixel -- a mask of what each photograph covers, clipped highlights, confidence --
    [L,1,H,W] / [B,L,1,H,W] or one plane for all shots, [1,1,H,W] / [B,1,1,H,W]: the loss is `(weights * (stack - photographs) ** 2).mean()`
    and the one-pass forms are the weighted ones (functional.rendering_loss_mse_stack(weights=))."""

    def __init__(self, light_type='point', view_dir=torch.tensor([0.0, 0.0, 1.0]), lights=torch.tensor([[0.1, 0.1, 1.0]]),
                 light_intensities=torch.tensor([1.0, 1.0, 1.0]), light_size=None, view_type='directional'):
        super().__init__()
        self.n_lights, self._rows = F_._stack_lights(lights, light_intensities)          # ValueError before any device work
        self._views = F_._stack_views(view_dir, self.n_lights)                           # 1, or L: one view per shot (a handheld capture)
        self.brdf = CookTorranceBRDF(light_type=light_type, view_type=view_type)         # 'point': `view_dir` is the camera's position
        self.view_dir = view_dir
        self.lights = lights
        self.light_intensities = light_intensities
        self.light_size = light_size

    def _kwargs(self, material):
        return dict(view_dir=self.view_dir, light=self.lights, light_intensity=self.light_intensities, light_type=self.brdf.light_type,
                    light_size=self.light_size, view_type=self.brdf.view_type, tile=material.lazy_tile, albedo_is_srgb=bool(material.albedo_is_srgb),
                    specular_is_srgb=bool(getattr(material, "specular_is_srgb", True)))

    def _render(self, material):
        """[L,3,H,W] / [B,L,3,H,W]: one launch where the maps can be read in place, else L calls of the BRDF module (CPU-resident maps,
        a lazy blend, maps not yet decoded: whatever the module handles)."""
        maps = _plain_maps(self.brdf, material)
        if maps is not None:
            return F_.cook_torrance_stack(*maps, **self._kwargs(material))
        lt = torch.as_tensor(self.lights, dtype=torch.float32).reshape(-1, 3)
        it = torch.as_tensor(self.light_intensities, dtype=torch.float32).reshape(-1, 3)
        vt = F_._view_rows(self.view_dir)
        return torch.stack([self.brdf(material, vt[l] if self._views > 1 else self.view_dir, lt[l], it[l if self._rows > 1 else 0], self.light_size)
                            for l in range(self.n_lights)], dim=-4)

    def forward(self, predicted_material, ground_truth, weights=None):
        """`ground_truth`: a material, or the stack of photographs ([L,3,H,W] / [B,L,3,H,W] tensor); `weights`: see the class."""
        targets = _reference(ground_truth, (self.view_dir, self.lights, self.light_intensities), self._render)
        maps = _plain_maps(self.brdf, predicted_material)
        if maps is None:
            rendered = self._render(predicted_material)
            if weights is not None:
                return F_._weighted_mse(rendered, targets, weights)
            return nn.MSELoss()(rendered, targets.to(rendered.device))
        return F_.rendering_loss_mse_stack(*maps, targets=targets.to(maps[0].device), **({} if weights is None else {"weights": weights}),
                                           **self._kwargs(predicted_material))
