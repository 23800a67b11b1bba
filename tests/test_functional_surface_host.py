"""pypbr_amd.functional is the namespace everything imports; its kernel families live in private sibling modules.  Every
name that resolved on it before the split still does -- private helpers included -- except the four settings that moved with the code
that reads them.

PARENT_NAMES was generated from the commit before the split, not written by hand, in a checkout of that commit:
    python -c "import types, pypbr_amd.functional as F; print(sorted(k for k, v in vars(F).items()
               if not (k.startswith('__') and k.endswith('__')) and not isinstance(v, types.ModuleType)))"
"""
from pypbr_amd import _dispatch, _upload
from pypbr_amd import functional as F

PARENT_NAMES = """
CACHING DEVICE_PARAMETERS ENCODED_DTYPES KeptPlan LAUNCHES Optional PADDING_MODES PINNED_RESULT_CAP PLANE_SKEW_BYTES PlaneMap RenderPlan
    RotatePlan STAGE_MEMCPY_LIMIT Sequence TensorLike Tuple UPLOAD_STAGE_CAP USE_TORCH_OPS Union ValueMemo VersionMemo _ColourFn _CookTorranceFn
    _DTYPES _DecodeNormalFn _FusedBlendFn _HOST_COPIES _LIGHT_TYPES _MetallicToSpecularFn _MseStepFn _NormalFromHeightFn _PARAM_KEYS _PINNED_OUT
    _PackFn _ROTATE_PLANS _RemapFn _ResizeFn _RotateFn _SpecularToMetallicFn _StepNotServed _TransformNormalsFn _UPLOAD_STAGE _UnpackFn
    _WARNED_PARAMETER_COPY _affine_plan _aligned_arena _as_batched _axis_map _blend_then_render_with_grad _colour_raw _cook_torrance_via_torch_op
    _decode_normal_raw _dense_samples _device_parameter_tensors _device_tensor _directx _ds2bm_raw _fused_blend_backward_can_take _grad_like
    _host_vec3 _m2ds_raw _make_rotate_plan _matrix _needs_grad _nfh_raw _on_device _pack _pack_material_major _pack_raw _page_locked_range
    _param_grad _param_tensor _pbr_map _plane_ops_call _plane_ptr _planes_of _remap_raw _resize_raw _rotate_geom _rotate_raw _rows_dense
    _run_plane_ops _stage_copy _staged _stream_ptr _torch_op_can_take _transform_raw _unpack_layout _unpack_raw _upload_stage _warn_parameter_copy
    build_descriptor check_crop cook_torrance decode_normal diffuse_specular_to_basecolor_metallic fold_stages host_values is_encoded linear_to_srgb
    metallic_to_diffuse_specular normal_from_height pack_maps pack_planes plan_cook_torrance refill_parameters release_upload_stage remap_planes
    rendering_loss_mse resize rotate_indices rotate_maps rotate_plan set_caching srgb_to_linear tile_counts to_host transform_normals unpack_image
    unpack_planes upload_packed version_of
""".split()

# The names functional has gained since the split (the light stacks, the height solve, the export path ...): the same command in a checkout of
# the commit before the loss steps were put on one frame, minus PARENT_NAMES.
GAINED_NAMES = """
STACK_LAUNCHES _HeightFromNormalFn _MseStackFitFn _MseStackStepFn _hfn_raw _poisson_solve _scale_step_gradients _stack_lights _stack_plain
    _stack_route cook_torrance_stack download_samples height_from_normal launch pack_image ptr rendering_loss_mse_stack
""".split()

MOVED_SETTINGS = ("PINNED_RESULT_CAP", "PLANE_SKEW_BYTES", "STAGE_MEMCPY_LIMIT", "UPLOAD_STAGE_CAP")


def test_every_name_of_the_parent_still_resolves_on_functional():
    assert len(PARENT_NAMES) == 122 and PARENT_NAMES == sorted(set(PARENT_NAMES))
    missing = [n for n in PARENT_NAMES if n not in MOVED_SETTINGS and not hasattr(F, n)]
    assert missing == []


def test_every_name_gained_since_the_split_still_resolves_on_functional():
    assert len(GAINED_NAMES) == 17 and GAINED_NAMES == sorted(set(GAINED_NAMES)) and not set(GAINED_NAMES) & set(PARENT_NAMES)
    assert {"STACK_LAUNCHES", "_MseStackStepFn", "_MseStackFitFn", "_stack_lights", "_stack_plain", "_stack_route", "_scale_step_gradients",
            "cook_torrance_stack", "rendering_loss_mse_stack"} <= set(GAINED_NAMES)
    missing = [n for n in GAINED_NAMES if not hasattr(F, n)]
    assert missing == []


def test_the_four_settings_live_on_the_module_that_reads_them_only():
    for name in MOVED_SETTINGS:
        assert name in PARENT_NAMES
        assert isinstance(getattr(_upload, name), int), name
        assert not hasattr(F, name), name        # a stale assignment on functional would bind a name nobody reads


def test_the_launch_counters_are_one_dict():
    assert F.LAUNCHES is _dispatch.LAUNCHES
    assert set(F.LAUNCHES) == {"remap_planes", "remap_planes_backward", "plane_ops", "plane_ops_backward", "rotate_planes", "rotate_planes_backward"}
