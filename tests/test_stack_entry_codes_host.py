"""The ORDER of the codes the twelve light-stack loss steps and the three fit-size queries return, host side (no device): a descriptor with two
faults gets the earlier check's code.  The per-family host tests pin one fault at a time; this one pins the sequence every entry point shares --
descriptor, the call's pointers, result dtype, what the family serves, the weights' shape -- so that the entry points cannot drift apart.
Every call here returns before anything is launched or read: the addresses are dummies."""
import ctypes

import pytest

from pypbr_amd import _native as N
from test_light_stack_host import _desc

STEPS = ["pbr_cook_torrance_%s%smse_stack_%s" % (family, weighted, step) for family in ("", "camera_", "view_")
         for weighted in ("", "weighted_") for step in ("step", "fit_step")]
SIZES = {"": "pbr_mse_stack_fit_workspace_bytes", "camera_": "pbr_camera_mse_stack_fit_workspace_bytes",
         "view_": "pbr_view_mse_stack_fit_workspace_bytes"}


def _family(name):
    return "view_" if "_view_" in name else "camera_" if "_camera_" in name else ""


def _call(name, d, targets=1, loss=1, workspace=1, g_params=1, weights=1, light_stride=None, host=1, device=0):
    """A loss step through ctypes: dummy non-NULL addresses, or NULL where the keyword says 0."""
    buf = (ctypes.c_float * 64)()
    at = lambda on: ctypes.addressof(buf) if on else None
    plane = d.height * d.width
    cams = ((buf if host else None), at(device)) if _family(name) == "view_" else ()
    beside = (at(weights), d.n_lights * plane, plane if light_stride is None else light_stride) if "weighted" in name else ()
    fit = (at(g_params),) if name.endswith("fit_step") else ()
    return getattr(N.lib(), name)(ctypes.byref(d), *cams, at(targets), *beside, None, None, None, None, None, *fit, at(loss), at(workspace), None)


def _size(family, d):
    return getattr(N.lib(), SIZES[family])(ctypes.byref(d))


def _f16(tile=(1, 1)):
    d = _desc(tile=tile)
    d.out_dtype = N.F16
    return d


def _nan_directional():
    d = _desc()
    d.light_type, d.light_size = N.LIGHT_DIRECTIONAL, float("nan")
    return d


def test_the_twelve_steps_are_bound():
    assert len(STEPS) == len(set(STEPS)) == 12 and all(s in N.EXPORTS for s in STEPS) and all(q in N.EXPORTS for q in SIZES.values())


@pytest.mark.parametrize("name", STEPS)
def test_a_descriptor_with_two_faults_gets_the_earlier_check_s_code(name):
    fit, weighted, view = name.endswith("fit_step"), "weighted" in name, _family(name) == "view_"
    # the descriptor before the call's pointers
    d = _desc()
    d.abi_version = 8
    assert _call(name, d, targets=0) == N.ERR_SHAPE
    # the call's pointers before the result's dtype
    for null in ("targets", "loss", "workspace"):
        assert _call(name, _f16(), **{null: 0}) == N.ERR_NULL_MAP, null
    if fit:
        assert _call(name, _f16(), g_params=0) == N.ERR_NULL_MAP
    if weighted:
        assert _call(name, _f16(), weights=0) == N.ERR_NULL_MAP
    if view:
        for host, device in ((0, 0), (1, 1)):                # exactly one source of positions
            assert _call(name, _f16(), host=host, device=device) == N.ERR_NULL_MAP
    # the result's dtype before what the family serves
    assert _call(name, _f16(tile=(2, 2))) == N.ERR_DTYPE
    # what the family serves before the weights' shape
    if weighted:
        assert _call(name, _desc(tile=(2, 2)), light_stride=1) == N.ERR_UNSUPPORTED
        assert _call(name, _desc(), light_stride=1) == N.ERR_SHAPE
    # a NaN grid: the camera's view vectors are NaN whatever the light type; a directional light never reads light_size otherwise
    if _family(name):
        assert _call(name, _nan_directional()) == N.ERR_UNSUPPORTED
    elif weighted:
        assert _call(name, _nan_directional(), light_stride=1) == N.ERR_SHAPE      # past the gate: the next check answers
    d = _desc()
    d.light_size = float("nan")                              # ... and the point light's grid is NaN in every family
    assert _call(name, d) == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("family", list(SIZES))
def test_a_size_query_is_zero_for_what_its_step_refuses(family):
    """Every fault that lies in the descriptor (not in the call's pointers): the fit step's code is not OK and the query says 0."""
    step = "pbr_cook_torrance_%smse_stack_fit_step" % family
    refused = []
    for field, value in (("abi_version", 8), ("width", 0), ("n_lights", 17), ("y_offset", -1), ("light_type", 7), ("workflow", 5),
                         ("out_dtype", N.F16), ("light_size", float("nan"))):
        d = _desc()
        setattr(d, field, value)
        refused.append((field, d))
    d = _desc()
    d.albedo.data = None
    refused += [("albedo", d), ("tiled", _desc(tile=(2, 2))), ("f16 and tiled", _f16(tile=(2, 2)))]
    if family:
        d = _desc()
        d.map_height, d.map_width = d.height_total, d.width  # map sizes set at all: the camera takes plain descriptors only
        refused += [("map size", d), ("nan directional", _nan_directional())]
    for what, d in refused:
        assert _call(step, d) != N.OK and _size(family, d) == 0, what
    assert _size(family, _desc()) > 0
    if not family:                                           # the orthographic forms do not refuse a NaN light_size beside a directional light
        assert _size(family, _nan_directional()) > 0
