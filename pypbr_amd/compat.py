"""Run reference scripts unchanged: `import pypbr_amd.compat; pypbr_amd.compat.install()` registers
`pypbr`, `pypbr.models`, `pypbr.materials`, `pypbr.utils`, `pypbr.io`, `pypbr.blending`, `pypbr.transforms` and
`pypbr.transforms.functional` as aliases of the pypbr_amd modules, so that e.g. examples/example_brdf.py's

    from pypbr.models import CookTorranceBRDF
    from pypbr.io import load_material_from_folder

resolve to the MI355X implementation.  The Cook-Torrance path and the calls either side of it
(load, blend, resize, tile) exist here, and so do the normal-map operations: `pypbr.utils.compute_normal_from_height`,
`rotate_normals`, `invert_normal` and the material methods `compute_normal_from_height`,
`adjust_normal_strength`, `invert_normal` resolve through the aliases above.  The geometric transforms exist too: the material
methods `crop` (in-bounds), `flip_horizontal`, `flip_vertical`, `roll`, and `pypbr.transforms` with upstream's classes and functional
forms, `Compose` running a chain of geometric stages as one kernel launch.  So do the packed-tensor methods `MaterialBase.from_tensor`,
`as_tensor` and `normal_rgb` (one kernel launch each).  Rotation exists as `pypbr_amd.rotation` (`rotate`, `random_rotate`, `Rotate`,
`RandomRotate`: one kernel launch per block of maps); the upstream NAMES `MaterialBase.rotate`, `transforms.Rotate` / `RandomRotate` and
`functional.rotate` / `random_rotate` do not resolve through the aliases yet.  The Poisson reconstruction of a height
map exists as `MaterialBase.compute_height_from_normal` and `pypbr_amd.functional.height_from_normal`; the function's upstream name
`pypbr.utils.compute_height_from_normal` does not resolve yet either.  Saving exists: `MaterialBase.to_pil`, `to_numpy`,
`save_to_folder` and `pypbr.io.save_material_to_folder` (the samples are made on the device, one kernel launch per map size).  Everything
else of PyPBR (out-of-bounds crops, ...) is out of scope and raises ImportError/AttributeError as an absent module would."""
import sys
import types


def install(force: bool = False) -> types.ModuleType:
    """Registers the aliases.  Refuses to shadow an already-imported real `pypbr` unless `force`."""
    import pypbr_amd
    from pypbr_amd import blending, io, materials, models, transforms, utils

    existing = sys.modules.get("pypbr")
    if existing is not None and not getattr(existing, "__pypbr_amd_alias__", False) and not force:
        raise RuntimeError("a different `pypbr` package is already imported from %s"
                           % getattr(existing, "__file__", "?"))
    pkg = types.ModuleType("pypbr")
    pkg.__doc__ = "alias of pypbr_amd (MI355X Cook-Torrance path)"
    pkg.__path__ = []                      # a package, with no files of its own
    pkg.__pypbr_amd_alias__ = True
    pkg.__version__ = pypbr_amd.__version__
    sys.modules["pypbr.blending.functional"] = blending
    sys.modules["pypbr.transforms.functional"] = transforms.functional
    for name, mod in (("models", models), ("materials", materials), ("utils", utils), ("io", io), ("blending", blending),
                      ("transforms", transforms)):
        setattr(pkg, name, mod)
        sys.modules["pypbr." + name] = mod
    sys.modules["pypbr"] = pkg
    return pkg


def uninstall() -> None:
    for name in [k for k, v in sys.modules.items() if k == "pypbr" or k.startswith("pypbr.")]:
        mod = sys.modules[name]
        if name == "pypbr" and not getattr(mod, "__pypbr_amd_alias__", False):
            return
        del sys.modules[name]
