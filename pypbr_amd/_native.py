"""ctypes binding of libpbr_hip.so (the C ABI declared in include/pbr_hip.h).

There is no Python/ATen fallback behind these calls: if the shared library is
missing, or no HIP device is present when a kernel has to run, the call raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBR_HIP_LIB") or os.path.join(_HERE, "libpbr_hip.so")   # env override: A/B of two builds

ABI_VERSION = 9
RESIZE_TWO_PASS, RESIZE_STRIP, RESIZE_TWO_TAP, RESIZE_BAND_WALK, RESIZE_ROW_WALK = range(5)      # pbr_resize_form
MAX_LIGHTS = 16

F32, F16 = 0, 1
LIGHT_DIRECTIONAL, LIGHT_POINT = 0, 1
WORKFLOW_METALLIC, WORKFLOW_SPECULAR, WORKFLOW_CONVERTED = 0, 1, 2
# (slots 0 and 4 are retired since ABI 8 -- PBR_TUNE_NONTEMPORAL, PBR_TUNE_BWD_VEC: their experiments are closed, the library ignores them)
(_TUNE_RESERVED_0, TUNE_BLOCK_LOG2, TUNE_F16_VEC, TUNE_LDS_BYTES, _TUNE_RESERVED_4, TUNE_BATCH_INNER, TUNE_SCALAR_BASE, TUNE_MAX_VEC, TUNE_BWD_RUN,
 TUNE_MSE_STREAM, TUNE_TILE_REPEAT, TUNE_RESIZE_UP2) = range(12)

TUNE_COUNT, TUNE_SLOTS, TUNE_UNSET = 12, 32, -2 ** 31
TUNE_NAMES = {"block_log2": TUNE_BLOCK_LOG2, "f16_vec": TUNE_F16_VEC, "lds_bytes": TUNE_LDS_BYTES, "batch_inner": TUNE_BATCH_INNER, "scalar_base": TUNE_SCALAR_BASE, "max_vec": TUNE_MAX_VEC,
              "bwd_run": TUNE_BWD_RUN, "mse_stream": TUNE_MSE_STREAM, "tile_repeat": TUNE_TILE_REPEAT, "resize_up2": TUNE_RESIZE_UP2}

OK = 0
ERR_NULL_MAP, ERR_WORKFLOW, ERR_LIGHT_TYPE, ERR_SHAPE, ERR_DTYPE, ERR_CHANNELS, ERR_NO_DEVICE = -1, -2, -3, -4, -5, -6, -7
ERR_UNSUPPORTED = -8

class PbrMap(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("batch_stride", ctypes.c_int64), ("channel_stride", ctypes.c_int64)]


class Tuning(ctypes.Structure):
    """pbr_tuning: per-call schedule knobs (PBR_TUNE_* index; TUNE_UNSET = the rule).  `Tuning.of(lds_bytes=0, ...)` builds one."""
    _fields_ = [("knob", ctypes.c_int32 * TUNE_SLOTS)]

    @classmethod
    def of(cls, **knobs):
        t = cls()
        for i in range(TUNE_SLOTS):
            t.knob[i] = TUNE_UNSET
        for name, value in knobs.items():
            t.knob[TUNE_NAMES[name]] = int(value)
        return t


class RenderDesc(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32), ("batch", ctypes.c_int32), ("height", ctypes.c_int32),
        ("width", ctypes.c_int32), ("height_total", ctypes.c_int32), ("y_offset", ctypes.c_int32),
        ("map_dtype", ctypes.c_int32), ("out_dtype", ctypes.c_int32), ("workflow", ctypes.c_int32),
        ("light_type", ctypes.c_int32), ("n_lights", ctypes.c_int32), ("albedo_is_srgb", ctypes.c_int32),
        ("specular_is_srgb", ctypes.c_int32), ("return_srgb", ctypes.c_int32),
        ("albedo", PbrMap), ("normal", PbrMap), ("roughness", PbrMap), ("metallic", PbrMap), ("specular", PbrMap),
        ("out", ctypes.c_void_p),
        ("view_dir", ctypes.c_float * 3), ("light_size", ctypes.c_float),
        ("lights", (ctypes.c_float * 3) * MAX_LIGHTS), ("intensities", (ctypes.c_float * 3) * MAX_LIGHTS),
        ("schedule", ctypes.c_int32), ("map_height", ctypes.c_int32), ("map_width", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("out_batch_stride", ctypes.c_int64), ("out_channel_stride", ctypes.c_int64),
        ("device_params", ctypes.c_void_p),
        ("tuning", ctypes.POINTER(Tuning)),
    ]


class BlendDesc(ctypes.Structure):
    """pbr_blend_desc: material 2 of a fused blend + the weights of material 1."""
    _fields_ = [("albedo", PbrMap), ("normal", PbrMap), ("roughness", PbrMap), ("metallic", PbrMap), ("specular", PbrMap),
                ("mask", PbrMap), ("sign_mode", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class MapGrads(ctypes.Structure):
    """pbr_map_grads: where the gradients of one material's maps go (NULL = not wanted)."""
    _fields_ = [("albedo", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("roughness", ctypes.c_void_p), ("metallic", ctypes.c_void_p),
                ("specular", ctypes.c_void_p)]


BLEND_SIGN_COMPUTE, BLEND_SIGN_GIVEN = 0, 1

PLANE_AFFINE, PLANE_NORMAL_XY = 0, 1
MAX_PLANE_OPS = 32


class PlaneOp(ctypes.Structure):
    """pbr_plane_op: one operation of a pbr_plane_ops / pbr_plane_ops_backward table (strides in elements)."""
    _fields_ = [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("src", ctypes.c_void_p), ("src_batch_stride", ctypes.c_int64), ("src_plane_stride", ctypes.c_int64),
                ("dst", ctypes.c_void_p), ("dst_batch_stride", ctypes.c_int64), ("dst_plane_stride", ctypes.c_int64),
                ("input", ctypes.c_void_p), ("input_batch_stride", ctypes.c_int64), ("input_plane_stride", ctypes.c_int64),
                ("scale", ctypes.c_float), ("bias", ctypes.c_float)]


MAX_IMAGE_PACKS = 8
MAX_RECTIFY_IMAGES = 16
MAX_PHOTOMETRIC_SHOTS = 16


class ImagePack(ctypes.Structure):
    """pbr_image_pack: one map of a pbr_pack_images table (strides in elements)."""
    _fields_ = [("src", ctypes.c_void_p), ("stride_c", ctypes.c_int64), ("stride_h", ctypes.c_int64), ("stride_w", ctypes.c_int64),
                ("dst", ctypes.c_void_p), ("channels", ctypes.c_int32), ("bits", ctypes.c_int32), ("encode_normal", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


ADAM_NONE, ADAM_BOX, ADAM_UNIT = 0, 1, 2
MAX_ADAM_TENSORS = 16
ADAM_BLOCK, ADAM_MAX_BLOCKS = 256, 1024      # PBR_ADAM_BLOCK, PBR_ADAM_MAX_BLOCKS: a lane loops on planes of more than 256 x 1024 quads


class AdamTensor(ctypes.Structure):
    """pbr_adam_tensor: one parameter of a pbr_adam_step table (strides in elements; m, v, master dense fp32)."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("master", ctypes.c_void_p), ("pixels", ctypes.c_int64),
                ("param_batch_stride", ctypes.c_int64), ("param_plane_stride", ctypes.c_int64),
                ("grad_batch_stride", ctypes.c_int64), ("grad_plane_stride", ctypes.c_int64),
                ("batch", ctypes.c_int32), ("channels", ctypes.c_int32), ("dtype", ctypes.c_int32), ("project", ctypes.c_int32),
                ("lo", ctypes.c_float), ("hi", ctypes.c_float), ("min_z", ctypes.c_float), ("group", ctypes.c_int32)]


class AdamCoeffs(ctypes.Structure):
    """pbr_adam_coeffs: what one group's step needs (a = lr / (1 - beta1^t), c = 1 / sqrt(1 - beta2^t))."""
    _fields_ = [("a", ctypes.c_float), ("c", ctypes.c_float), ("one_minus_beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("one_minus_beta2", ctypes.c_float), ("eps", ctypes.c_float)]


class AdamGroup(ctypes.Structure):
    """pbr_adam_group: one row of pbr_adam_advance (a DEVICE float counter; lr from the host value or a DEVICE float)."""
    _fields_ = [("step", ctypes.c_void_p), ("lr_device", ctypes.c_void_p), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double)]


SMOOTH_L2, SMOOTH_CHARBONNIER = 0, 1
MAX_SMOOTH_TENSORS = 8
SMOOTH_BLOCK, SMOOTH_BAND_ROWS = 256, 32     # PBR_SMOOTH_BLOCK, PBR_SMOOTH_BAND_ROWS: 4 waves of 63 units + 1 halo unit; rows of a band at the most
SMOOTH_MIN_BAND_ROWS, SMOOTH_MIN_BLOCKS = 4, 512      # ... halved down to 4 while a launch has fewer than 512 workgroups


class SmoothTensor(ctypes.Structure):
    """pbr_smooth_tensor: one map of a pbr_smoothness_step table (strides in elements; grad NULL: value only; weights NULL: 1)."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("weights", ctypes.c_void_p),
                ("param_batch_stride", ctypes.c_int64), ("param_plane_stride", ctypes.c_int64),
                ("grad_batch_stride", ctypes.c_int64), ("grad_plane_stride", ctypes.c_int64), ("weights_batch_stride", ctypes.c_int64),
                ("k", ctypes.c_double), ("eps", ctypes.c_float), ("dtype", ctypes.c_int32),
                ("batch", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("kind", ctypes.c_int32), ("wrap", ctypes.c_int32)]


class RotateGeom(ctypes.Structure):
    """pbr_rotate_geom: the host-computed constants of one rotation (functional.rotate_plan)."""
    _fields_ = [("pad", ctypes.c_int32), ("circular", ctypes.c_int32), ("x0", ctypes.c_float), ("y0", ctypes.c_float),
                ("t00", ctypes.c_float), ("t10", ctypes.c_float), ("t01", ctypes.c_float), ("t11", ctypes.c_float),
                ("cos_r", ctypes.c_float), ("sin_r", ctypes.c_float)]


SCHEDULE_AUTO, SCHEDULE_LINEAR = 0, 1


def schedule_xcd(c: int) -> int:
    """PBR_SCHEDULE_XCD(c): every XCD takes runs of 1 << c consecutive tiles."""
    return 1 + c


# header struct name -> its ctypes mirror (tests/test_abi_binding_host.py compares sizes, field offsets and field sizes with a C compiler's)
STRUCTS = {
    "pbr_map": PbrMap, "pbr_tuning": Tuning, "pbr_render_desc": RenderDesc, "pbr_blend_desc": BlendDesc, "pbr_map_grads": MapGrads,
    "pbr_rotate_geom": RotateGeom, "pbr_plane_op": PlaneOp, "pbr_image_pack": ImagePack, "pbr_adam_tensor": AdamTensor,
    "pbr_adam_coeffs": AdamCoeffs, "pbr_adam_group": AdamGroup, "pbr_smooth_tensor": SmoothTensor,
}

_int, _i32, _i64, _u32, _sz = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_size_t
_f32, _vp, _str = ctypes.c_float, ctypes.c_void_p, ctypes.c_char_p
_fp = ctypes.POINTER(ctypes.c_float)                 # a HOST float array (a void pointer where the header's float * is device memory)
_desc, _blend, _grads = ctypes.POINTER(RenderDesc), ctypes.POINTER(BlendDesc), ctypes.POINTER(MapGrads)
_geom, _smooth, _adam = ctypes.POINTER(RotateGeom), ctypes.POINTER(SmoothTensor), ctypes.POINTER(AdamTensor)

# THE binding: one row per entry point of include/pbr_hip.h -- name: (return type, [argument types, in the header's order]) -- in the order
# of the header, the light-stack loss steps excepted (generated below).  lib() applies it; tests/test_abi_binding_host.py checks the function
# objects lib() hands out, row by row, against the header's prototypes.  A new entry point: its prototype there, its row here.
SIGNATURES = {
    "pbr_tuning_init": (None, [ctypes.POINTER(Tuning)]),
    "pbr_cook_torrance": (_int, [_desc, _vp]),
    "pbr_cook_torrance_autotune": (_int, [_desc, _vp, ctypes.POINTER(_i32)]),
    "pbr_blend_normal_sign": (_int, [_desc, _blend, _vp, _vp]),
    "pbr_cook_torrance_blend": (_int, [_desc, _blend, _vp, _vp]),
    "pbr_blend_backward_serves": (_int, [_desc]),
    "pbr_cook_torrance_blend_backward": (_int, [_desc, _blend, _vp, _vp, _grads, _grads, _vp, _vp]),
    "pbr_cook_torrance_backward": (_int, [_desc] + [_vp] * 7),
    "pbr_backward_folded_workspace_bytes": (_sz, [_desc]),
    "pbr_cook_torrance_backward_folded": (_int, [_desc] + [_vp] * 8),
    "pbr_param_grad_workspace_bytes": (_sz, [_desc]),
    "pbr_cook_torrance_backward_params": (_int, [_desc] + [_vp] * 9),
    "pbr_mse_step_workspace_bytes": (_sz, [_desc]),
    "pbr_cook_torrance_mse_step": (_int, [_desc] + [_vp] * 9),
    "pbr_cook_torrance_stack": (_int, [_desc, _vp]),
    "pbr_cook_torrance_camera": (_int, [_desc, _vp]),
    "pbr_camera_backward_workspace_bytes": (_sz, [_desc]),
    "pbr_cook_torrance_camera_backward": (_int, [_desc] + [_vp] * 9),
    "pbr_cook_torrance_camera_stack": (_int, [_desc, _vp]),
    # one camera position per shot: (desc, cameras_host float[L][3] | NULL, cameras_device | NULL, ...) -- exactly one of the two
    "pbr_cook_torrance_view_stack": (_int, [_desc, _fp, _vp, _vp]),
    "pbr_device_params_bytes": (_sz, []),
    "pbr_prepare_device_params": (_int, [_desc, _vp, _vp, _vp, _i32, _vp, _vp]),
    "pbr_scale_by_device_scalar": (_int, [_vp, _sz, _int, _vp, _vp]),
    "pbr_scale_list_by_device_scalar": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_sz), _int, _int, _vp, _vp]),
    "pbr_srgb_to_linear": (_int, [_vp, _vp, _sz, _int, _vp]),
    "pbr_linear_to_srgb": (_int, [_vp, _vp, _sz, _int, _vp]),
    "pbr_metallic_to_specular": (_int, [_vp, _vp, _vp, _vp, _i32, _i64, _int, _int, _vp]),
    "pbr_specular_to_metallic": (_int, [_vp, _vp, _vp, _vp, _sz, _int, _int, _vp]),
    "pbr_srgb_to_linear_backward": (_int, [_vp, _vp, _vp, _sz, _int, _vp]),
    "pbr_linear_to_srgb_backward": (_int, [_vp, _vp, _vp, _sz, _int, _vp]),
    "pbr_metallic_to_specular_backward": (_int, [_vp] * 6 + [_i32, _i64, _int, _int, _vp]),
    "pbr_specular_to_metallic_backward": (_int, [_vp] * 6 + [_sz, _int, _int, _vp]),
    "pbr_decode_normal_backward": (_int, [_vp, _vp, _vp, _i32, _i64, _vp, _vp]),
    "pbr_fold_gradient": (_int, [_vp, _vp] + [_i32] * 6 + [_int, _vp]),
    "pbr_fold_gradient_typed": (_int, [_vp, _vp] + [_i32] * 6 + [_int, _int, _vp]),
    "pbr_decode_normal": (_int, [_vp, _vp, _i32, _i64, _int, _vp, _vp]),
    "pbr_normal_from_height": (_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _f32, _i32, _int, _vp]),
    "pbr_normal_from_height_backward": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp]),
    "pbr_normal_transform": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i64, _f32, _f32, _f32, _f32, _i32, _int, _vp]),
    "pbr_normal_transform_backward": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i64, _f32, _f32, _f32, _f32, _i32, _vp]),
    "pbr_normal_divergence": (_int, [_vp, _i64, _i64, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _int, _vp]),
    "pbr_normal_divergence_backward": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _f32, _i32, _vp]),
    "pbr_poisson_scale": (_int, [_vp, _i64, _i32, _i32, _i32, _vp]),
    "pbr_height_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "pbr_height_stats": (_int, [_vp, _i64, _vp, _i32, _i32, _i32, _vp]),
    "pbr_height_normalize": (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _int, _vp]),
    "pbr_height_normalize_backward": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "pbr_remap_planes": (_int, [_vp, _i64, _i64, _vp, _i64, _i64] + [_i32] * 10 + [_u32, _int, _vp]),
    "pbr_remap_planes_backward": (_int, [_vp, _i64, _i64, _vp, _i64, _i64] + [_i32] * 10 + [_u32, _vp]),
    "pbr_rotate_planes": (_int, [_vp, _i64, _i64, _vp, _i64, _i64] + [_i32] * 6 + [_geom, _i32, _f32, _f32, _f32, _f32, _int, _vp]),
    "pbr_rotate_planes_backward": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64] + [_i32] * 6
                                   + [_geom, _i32, _f32, _f32, _f32, _f32, _vp]),
    "pbr_plane_ops": (_int, [ctypes.POINTER(PlaneOp), _i32, _i32, _i64, _int, _vp]),
    "pbr_plane_ops_backward": (_int, [ctypes.POINTER(PlaneOp), _i32, _i32, _i64, _int, _vp]),
    "pbr_unpack_image": (_int, [_vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _vp, _i32, _vp]),
    "pbr_pack_images": (_int, [ctypes.POINTER(ImagePack), _i32, _i32, _i32, _vp]),
    # (src, n_images, src_height, src_width, image / row / pixel / channel stride in samples, HOST homographies double[n][9], targets, weights,
    #  height, width, supersample, clip_level, to_linear, stream)
    "pbr_rectify_images": (_int, [_vp, _i32, _i32, _i32, _i64, _i64, _i64, _i64, ctypes.POINTER(ctypes.c_double), _vp, _vp,
                                  _i32, _i32, _i32, _i32, _i32, _vp]),
    # (targets, weights | NULL, weights_shared, n_shots, height, width, HOST lights float[L][3], HOST intensities float[L][3], light_type,
    #  light_size, targets_srgb, iterations, shadow_cos, min_condition, albedo_srgb, normal, albedo, confidence, stream)
    "pbr_photometric_stereo": (_int, [_vp, _vp, _i32, _i32, _i32, _i32, _fp, _fp, _i32, _f32, _i32, _i32, _f32, _f32, _i32,
                                      _vp, _vp, _vp, _vp]),
    "pbr_resize_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "pbr_resize_bilinear": (_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _int, _vp, _vp]),
    "pbr_resize_form": (_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _int, _vp]),
    "pbr_resize_backward_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "pbr_resize_bilinear_backward": (_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _int, _vp, _vp]),
    "pbr_blend_maps": (_int, [_vp, _vp, _vp, _vp, _i32, _i64, _int, _vp]),
    "pbr_blend_maps_backward": (_int, [_vp] * 7 + [_i32, _i64, _int, _int, _vp]),
    "pbr_blend_sigmoid_mask": (_int, [_vp, _vp, _vp, _i64, _f32, _f32, _vp]),
    "pbr_blend_sigmoid_mask_backward": (_int, [_vp, _vp, _vp, _vp, _i64, _f32, _vp]),
    "pbr_blend_gradient_mask": (_int, [_vp, _i32, _i32, _int, _vp]),
    "pbr_adam_step": (_int, [_adam, _i32, ctypes.POINTER(AdamCoeffs), _vp, _i32, _vp]),
    "pbr_adam_check": (_int, [_adam, _i32, _i32]),
    "pbr_adam_tensor_size": (_sz, []),
    "pbr_adam_advance": (_int, [ctypes.POINTER(AdamGroup), _i32, _vp, _vp]),
    "pbr_smoothness_step": (_int, [_smooth, _i32, _vp, _vp, _vp, _sz, _vp]),
    "pbr_smoothness_workspace_bytes": (_sz, [_smooth, _i32]),
    "pbr_smoothness_check": (_int, [_smooth, _i32]),
    "pbr_smooth_tensor_size": (_sz, []),
    "pbr_abi_version": (_int, []),
    "pbr_build_id": (_str, []),
    "pbr_render_desc_size": (_sz, []),
    "pbr_error_string": (_str, [_int]),
    "pbr_kernel_name": (_str, [_desc]),
    "pbr_bytes_per_pixel": (_int, [_desc]),
    "pbr_set_tuning": (_int, [_int, _int]),
}
# the twelve light-stack loss steps: (desc, [the shots' cameras,] targets, [weights, w_batch_stride, w_light_stride,] g_* (5), [g_params,]
# loss, workspace, stream), and the three families' fit-size queries
for _family, _before in (("", []), ("camera_", []), ("view_", [_fp, _vp])):
    for _weighted, _beside in (("", []), ("weighted_", [_vp, _i64, _i64])):
        for _step, _pointers in (("step", 8), ("fit_step", 9)):
            SIGNATURES["pbr_cook_torrance_%s%smse_stack_%s" % (_family, _weighted, _step)] = (
                _int, [_desc] + _before + [_vp] + _beside + [_vp] * _pointers)
    SIGNATURES["pbr_%smse_stack_fit_workspace_bytes" % _family] = (_sz, [_desc])

EXPORTS = tuple(SIGNATURES)          # every symbol include/pbr_hip.h declares


class NativeLibraryError(RuntimeError):
    pass


_lib = None


def lib():
    """Loads libpbr_hip.so once and gives every entry point the types of its SIGNATURES row.  torch is imported first so that the
    process keeps ONE HIP runtime (torch's bundled libamdhip64.so.7; ours has the same soname)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (loads libamdhip64 before our library asks for it)
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C pypbr_amd/csrc`.  pypbr_amd has no CPU fallback." % LIB_PATH)
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise NativeLibraryError("cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    for c_name, cls in STRUCTS.items():      # the structs whose compiled size the library tells
        if c_name + "_size" in SIGNATURES and getattr(L, c_name + "_size")() != ctypes.sizeof(cls):
            raise NativeLibraryError("%s layout mismatch: library %d bytes, binding %d"
                                     % (c_name, getattr(L, c_name + "_size")(), ctypes.sizeof(cls)))
    if L.pbr_abi_version() != ABI_VERSION:
        raise NativeLibraryError("libpbr_hip.so ABI %d, binding expects %d" % (L.pbr_abi_version(), ABI_VERSION))
    for env, knob in tuple(("PBR_TUNE_" + name.upper(), index) for name, index in TUNE_NAMES.items()):      # profiling runs: knobs from the environment
        if os.environ.get(env, "") != "":
            L.pbr_set_tuning(knob, int(os.environ[env]))
    _lib = L
    return L


def source_hash():
    """The digest pbr_build_id() would return for the sources next to this package (the Makefile's recipe: sorted csrc/*.hip and *.hpp,
    include/pbr_hip.h, the Makefile), or None where the sources are not shipped."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")))
    files += [os.path.join(_HERE, "..", "include", "pbr_hip.h"), os.path.join(csrc, "Makefile")]
    if not files or not all(os.path.isfile(f) for f in files):
        return None
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_stamp() -> dict:
    """What every evidence file says about the binary it measured: the commit (PBR_GIT_HEAD in the environment -- the GPU box has no
    .git -- else `git rev-parse HEAD`), the library's own SHA-256, the digest of the sources it was built from (compiled in) and
    whether that is still the digest of the sources on disk (`stale`: the library would not be what `make` builds now)."""
    import hashlib
    import subprocess
    head = os.environ.get("PBR_GIT_HEAD")
    if not head:
        try:
            root = os.path.dirname(_HERE)
            head = subprocess.check_output(["git", "-C", root, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
            if subprocess.check_output(["git", "-C", root, "status", "--porcelain", "--untracked-files=no"], stderr=subprocess.DEVNULL).strip():
                head += "+uncommitted"
        except Exception:  # noqa: BLE001
            head = "unknown"
    with open(LIB_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    built_from, now = lib().pbr_build_id().decode(), source_hash()
    return {"git_head": head, "libpbr_hip_sha256": sha, "built_from_sources": built_from, "sources_on_disk": now,
            "stale": now is not None and now != built_from}


def error_string(code: int) -> str:
    return lib().pbr_error_string(code).decode()


def check(code: int):
    """Maps C-ABI status codes onto the exceptions the reference raises for the same
    condition (cooktorrance.py:62-65, :115-118; base.py:219)."""
    if code == OK:
        return
    msg = error_string(code)
    if code in (ERR_WORKFLOW, ERR_LIGHT_TYPE, ERR_CHANNELS, ERR_SHAPE, ERR_NULL_MAP):
        raise ValueError(msg)
    if code == ERR_DTYPE:
        raise TypeError(msg)
    if code == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError("HIP error %d: %s" % (code, msg))


def require_device():
    """The product has no CPU path: anything that computes needs a ROCm device."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("pypbr_amd needs a ROCm/HIP device (MI355X); there is no CPU fallback")
