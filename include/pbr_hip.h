/*
 * pbr_hip.h -- C ABI of libpbr_hip.so: fused Cook-Torrance evaluation of PBR
 * material maps on AMD MI355X (gfx950), plus the map conversions the path pulls in.
 *
 * This is the drop-in boundary of the build.  The reference
 * (giuvecchio/PyPBR) has no FFI: its hot path sits behind a Python callable,
 *     pypbr.models.CookTorranceBRDF.forward      pypbr/models/cooktorrance.py:68-182
 * and the entry points below are what a native binding for that path binds
 * (INTEGRATION.md shows the ctypes stub a PyPBR maintainer would add).  Plain
 * pointers and sizes only -- no torch types.  All map pointers are DEVICE pointers;
 * light/view parameters are HOST values (they travel in the kernel-argument
 * segment, i.e. in SGPRs: the wave-uniform broadcast is free).
 *
 * Threading: every call only enqueues work on `stream` (a hipStream_t passed as
 * void*, NULL = the null stream); no call synchronises with the host or allocates
 * device memory, and a call's behaviour is a function of its arguments (same
 * contract as the reference: synchronous-looking, stateless, re-entrant) -- with ONE
 * documented exception: pbr_set_tuning below is a process-global test / bench /
 * profiling hook (atomic words) that changes which schedule later calls of the whole
 * process pick.  Results never depend on it, only speed; product code leaves it alone
 * and passes per-call settings through pbr_render_desc.tuning instead.  Inputs are
 * never written.
 *
 * Map layout (pypbr/materials/base.py: maps are (C,H,W) float32, channel-first):
 * planar [B][C][H][W], rows contiguous (row stride == width).  `batch_stride`
 * and `channel_stride` are in ELEMENTS, so a row band of a taller map, or one
 * map shared by the whole batch (batch_stride = 0), is passed without a copy.
 */
#ifndef PBR_HIP_H
#define PBR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBR_HIP_ABI_VERSION 9      /* 9: the normal-map operations (pbr_normal_from_height, pbr_normal_transform and their gradients); 8: pbr_cook_torrance_blend_backward over tiled maps (map-sized gradients), pbr_blend_backward_serves; 7: folded gradients of tiled maps (pbr_cook_torrance_backward_folded), the loss step over tiled maps, 12 schedule knobs (was 23); 6: pbr_render_desc.tuning (per-call schedule knobs; pbr_set_tuning demoted to a process-global test hook); 5: pbr_render_desc.device_params (view / light / intensity read from device memory); 4: light_size follows Python truthiness, gradients of the map ops */
#define PBR_MAX_LIGHTS 16

/* ---- status codes (negative = caller error, positive = HIP runtime error code + 1000) */
enum {
    PBR_OK = 0,
    PBR_ERR_NULL_MAP = -1,        /* a required map pointer is NULL */
    PBR_ERR_WORKFLOW = -2,        /* neither metallic nor specular: cooktorrance.py:115-118 ValueError */
    PBR_ERR_LIGHT_TYPE = -3,      /* cooktorrance.py:62-65 ValueError */
    PBR_ERR_SHAPE = -4,           /* non-positive extent, band outside the map, > PBR_MAX_LIGHTS */
    PBR_ERR_DTYPE = -5,
    PBR_ERR_CHANNELS = -6,        /* base.py:219 "Normal map must have 2 or 3 channels." */
    PBR_ERR_NO_DEVICE = -7,
    PBR_ERR_UNSUPPORTED = -8      /* valid request this build does not implement */
};

enum { PBR_F32 = 0, PBR_F16 = 1 };                 /* storage type of maps */
enum { PBR_LIGHT_DIRECTIONAL = 0, PBR_LIGHT_POINT = 1 };   /* cooktorrance.py:61-65 */
enum {
    PBR_WORKFLOW_METALLIC = 0,    /* BasecolorMetallicMaterial: cooktorrance.py:103-107 */
    PBR_WORKFLOW_SPECULAR = 1,    /* DiffuseSpecularMaterial:   cooktorrance.py:108-114 */
    PBR_WORKFLOW_CONVERTED = 2    /* metallic maps, converted in-kernel by
                                     to_diffuse_specular_material (metallic.py:71-120),
                                     rendered in the specular workflow (config 3) */
};

typedef struct pbr_map {
    const void *data;             /* device pointer, NULL = map absent */
    int64_t batch_stride;         /* elements between materials */
    int64_t channel_stride;       /* elements between channel planes */
} pbr_map;

/* ---- schedule knobs ------------------------------------------------------------------
 * HOW a launch is scheduled (never WHAT it computes: every setting gives bit-identical results).  Each knob has a built-in rule
 * (measured on MI355X); a caller that knows better passes a pbr_tuning with the descriptor -- per call, caller-owned,
 * nothing outlives the call.  Entries left at PBR_TUNE_UNSET follow the rule (or the process-wide test hook pbr_set_tuning). */
enum {
    PBR_TUNE_RESERVED_0 = 0,            /* (ABI <= 7: PBR_TUNE_NONTEMPORAL.  The streaming hints are rules since ABI 8 -- on for vector lanes, stores only in the repeat-inner kernels --
                                           and the instantiations only this knob reached are not built; the slot is ignored) */
    PBR_TUNE_BLOCK_LOG2 = 1,            /* workgroup = 1 << value lanes (6..8); 0 = rule */
    PBR_TUNE_F16_VEC = 2,               /* pixels per lane for fp16 maps (4 | 8) */
    PBR_TUNE_LDS_BYTES = 3,             /* unused dynamic LDS per workgroup of the render kernel: an occupancy governor (-1 = rule) */
    PBR_TUNE_RESERVED_4 = 4,            /* (ABI <= 7: PBR_TUNE_BWD_VEC.  Pixels per lane of the backward kernels are a rule since ABI 8; ignored) */
    PBR_TUNE_BATCH_INNER = 5,           /* several lights: materials per lane of the batch-inner kernel (-1 = rule, 0 = one-material kernel) */
    PBR_TUNE_SCALAR_BASE = 6,           /* scalar plane addresses: 0 never, 1 rule (single materials), 2 whenever the launch allows them */
    PBR_TUNE_MAX_VEC = 7,               /* at most this many pixels per lane (8 default; 1 = the one-pixel kernels everywhere) */
    PBR_TUNE_BWD_RUN = 8,               /* rounds of the streamed backward kernel for fp16 maps with one light (-1 = rule, 0 = the one-tile kernels) */
    PBR_TUNE_MSE_STREAM = 9,            /* rendering-loss step for fp16 maps with one light: the streamed kernel (1, default) or the one-tile kernels (0) */
    PBR_TUNE_TILE_REPEAT = 10,          /* tiled maps: every texel loaded and decoded once and evaluated / differentiated at all its repeats (-1 = rule: on, 0 = wrap-around addressing, gradients folded by a second kernel) */
    PBR_TUNE_RESIZE_UP2 = 11,           /* the register-only resize kernels -- two taps for up-scales on both axes, the band walk for whole factors 2 ... 8 | 16 down, the row walk for other antialiased down-scales from 7 x up (1, default) -- or the strip kernels (0); 2 = as 1, with the row walk at every antialiased down-scale it can take (a test / measurement setting) */
    PBR_TUNE_COUNT = 12
};
/* (10 knobs in use since ABI 8.  ABI 6 carried 23 knobs; the 11 whose experiments are closed -- workgroup interleave, 16-byte streamed backward, the resize
 * kernels' row / tile-order / quad-store / gradient-form switches, the map kernels' launch shape, the wrap-around fold order, packed
 * one-light arithmetic, the XCD run length that pbr_render_desc.schedule already carries -- are rules now: profiles/EXPERIMENTS.md.) */
#define PBR_TUNE_UNSET INT32_MIN
#define PBR_TUNE_SLOTS 32               /* room for knobs of later versions: a pbr_tuning never changes size */
typedef struct pbr_tuning {
    int32_t knob[PBR_TUNE_SLOTS];       /* indexed by PBR_TUNE_*; PBR_TUNE_UNSET = no opinion.  Initialise with pbr_tuning_init */
} pbr_tuning;
/* Sets every entry to PBR_TUNE_UNSET. */
void pbr_tuning_init(pbr_tuning *t);

/*
 * One evaluation = CookTorranceBRDF.forward for `batch` materials and `n_lights`
 * lights.  Replaces cooktorrance.py:92-182 plus the lazy conversions it calls:
 * MaterialBase.linear_albedo (base.py:262-277), DiffuseSpecularMaterial.linear_specular
 * (diffuse.py:76-91), utils.srgb_to_linear / linear_to_srgb (utils/functions.py:31-66).
 */
typedef struct pbr_render_desc {
    int32_t abi_version;          /* PBR_HIP_ABI_VERSION */
    int32_t batch;                /* B >= 1.  The reference is unbatched (B = 1); B > 1 == a loop of calls */
    int32_t height;               /* rows of this band */
    int32_t width;                /* W */
    int32_t height_total;         /* rows of the full map: the point-light y grid spans it (cooktorrance.py:133) */
    int32_t y_offset;             /* first row of the band inside the full map (0 for a whole map) */

    int32_t map_dtype;            /* PBR_F32 | PBR_F16: albedo/normal/roughness/metallic/specular */
    int32_t out_dtype;            /* PBR_F32 | PBR_F16 */
    int32_t workflow;             /* PBR_WORKFLOW_* */
    int32_t light_type;           /* PBR_LIGHT_* */
    int32_t n_lights;             /* L in [1, PBR_MAX_LIGHTS]; L > 1: per-light clamp, sum, clamp, encode */
    int32_t albedo_is_srgb;       /* MaterialBase.albedo_is_srgb (base.py:72) */
    int32_t specular_is_srgb;     /* DiffuseSpecularMaterial.specular_is_srgb (diffuse.py:64);
                                     CONVERTED: 1 reproduces the upstream default of the converted
                                     material (already-linear specular decoded again), 0 = decoded once */
    int32_t return_srgb;          /* forward(..., return_srgb) cooktorrance.py:179-180 */

    pbr_map albedo;               /* 3 channels, required */
    pbr_map normal;               /* 3 channels, decoded to [-1,1]; data NULL = +Z (cooktorrance.py:147-152) */
    pbr_map roughness;            /* 1 channel, required */
    pbr_map metallic;             /* 1 channel: METALLIC / CONVERTED */
    pbr_map specular;             /* 3 channels: SPECULAR */
    void *out;                    /* [B][3][height][width]; contiguous unless out_*_stride (below) say otherwise */

    float view_dir[3];            /* un-normalised, as handed to forward (normalised like F.normalize, :95) */
    float light_size;             /* point lights; `light_size or 1.0` (cooktorrance.py:130) is Python truthiness: 0 (None upstream)
                                     means 1.0; a negative size mirrors the grid and NaN makes every result NaN, as upstream */
    float lights[PBR_MAX_LIGHTS][3];       /* direction (normalised here, :126) or position (:129) */
    float intensities[PBR_MAX_LIGHTS][3];  /* light_intensity per light (:96) */

    int32_t schedule;             /* workgroup -> tile order: PBR_SCHEDULE_AUTO (built-in rule), PBR_SCHEDULE_LINEAR, or
                                     PBR_SCHEDULE_XCD(c): every XCD takes runs of 1 << c consecutive tiles.  Results do
                                     not depend on it (bit-identical); pbr_cook_torrance_autotune measures the best */
    int32_t map_height;           /* MaterialBase.tile (base.py:524-537) fused as wrap-around addressing: when both are */
    int32_t map_width;            /* non-zero the maps are [B][C][map_height][map_width] and repeat over the
                                     height_total x width output (both must divide it); texel of output pixel (y, x)
                                     = ((y_offset + y) mod map_height, x mod map_width).  The point-light grid spans
                                     the OUTPUT, as it does after the reference's tile().  0/0: maps are output-sized */
    int32_t reserved;             /* 0 */
    int64_t out_batch_stride;     /* elements between the results of consecutive materials; 0 = 3 * height * width */
    int64_t out_channel_stride;   /* elements between the result's channel planes; 0 = height * width (contiguous).
                                     Rows are always contiguous.  Lets the result of material b sit right behind its
                                     maps ("material-major" batches) */
    const void *device_params;    /* NULL: view_dir / lights / intensities above are used.  Else a block of pbr_device_params_bytes() bytes
                                     written by pbr_prepare_device_params (earlier on the same stream): the kernels read view, light and
                                     intensity from it -- parameters that live in device memory (a light being fitted: cooktorrance.py:95-96,
                                     :126-140 are torch ops on device tensors upstream) never travel through the host, so a step neither
                                     synchronises nor bakes their values into a captured graph.  n_lights still counts the rows */
    const pbr_tuning *tuning;     /* NULL: the built-in rules.  Else per-call schedule knobs (above), read during the call only */
} pbr_render_desc;

#define PBR_SCHEDULE_AUTO 0
#define PBR_SCHEDULE_LINEAR 1
#define PBR_SCHEDULE_XCD(c) (1 + (c))     /* c in [1, 12] */

/* Enqueue the fused kernel.  Returns PBR_OK or an error code; never blocks. */
int pbr_cook_torrance(const pbr_render_desc *desc, void *stream);

/*
 * Which HBM channels the 8 + 3 plane streams of a launch land on depends on the buffers' addresses and
 * strides, and so does the better workgroup order (measured spread between the two orders: -6 ... +14 %).
 * Times the candidate schedules on the descriptor's own buffers (a few launches each, `out` is rewritten
 * with the same values), BLOCKS until they are done, and stores the fastest in *schedule for the caller to put
 * into desc->schedule.  Optional: PBR_SCHEDULE_AUTO picks by a rule derived from the same measurements.
 */
int pbr_cook_torrance_autotune(const pbr_render_desc *desc, void *stream, int32_t *schedule);

/*
 * Material blending fused in front of the evaluation: what examples/example_blend.py:14-32 does with
 * blend_with_mask (pypbr/blending/functional.py:64-145: every map mask*map1 + (1-mask)*map2, normals normalised,
 * blended, normalised), the re-assignment of the blended normal map (MaterialBase._process_normal_map again,
 * base.py:191-242) and CookTorranceBRDF.forward, in one pass: both materials are read once and the blended
 * maps are never written.  `desc` describes material 1 and the evaluation exactly as for pbr_cook_torrance;
 * `blend` holds material 2 (same dtype -- fp32 only --, workflow and extent; all of albedo, normal, roughness and
 * metallic|specular present in both) and the weights of material 1.  `workspace`: `batch` ints of device memory,
 * one "the blended normal map has a negative component" flag per material (base.py:212: a property of the WHOLE map).
 * sign_mode PBR_BLEND_SIGN_COMPUTE: a first small kernel on `stream` sets the flags from the maps the descriptor
 * holds -- whole maps only (a row band of an untiled map returns PBR_ERR_UNSUPPORTED).  PBR_BLEND_SIGN_GIVEN: the
 * caller has filled `workspace`, e.g. for row bands (multi-GPU sharding of one material): zero it, run
 * pbr_blend_normal_sign on every band (it only ever sets flags), combine the bands' flags (MAX), then evaluate.
 */
enum { PBR_BLEND_SIGN_COMPUTE = 0, PBR_BLEND_SIGN_GIVEN = 1 };
typedef struct pbr_blend_desc {
    pbr_map albedo, normal, roughness, metallic, specular;   /* material 2 */
    pbr_map mask;                 /* 1 channel fp32 in [0,1], [B|1][map rows][map cols]; batch_stride 0 = shared */
    int32_t sign_mode;            /* PBR_BLEND_SIGN_* */
    int32_t reserved;             /* 0 */
} pbr_blend_desc;
int pbr_blend_normal_sign(const pbr_render_desc *desc, const pbr_blend_desc *blend, void *workspace, void *stream);
int pbr_cook_torrance_blend(const pbr_render_desc *desc, const pbr_blend_desc *blend, void *workspace, void *stream);

/*
 * Gradient of pbr_cook_torrance_blend w.r.t. BOTH materials and the mask, in one pass (what autograd derives from
 * examples/example_blend.py:14-32 inside a rendering loss: CookTorranceBRDF.forward, the re-assignment of the blended normal
 * base.py:191-242, blend_with_mask blending/functional.py:64-145).  `desc` / `blend` / `workspace` exactly as for the forward
 * call (PBR_BLEND_SIGN_COMPUTE recomputes the flags; row bands need PBR_BLEND_SIGN_GIVEN); `grad_out` [B][3][H][W] fp32
 * contiguous.  Every non-NULL member of g_material1 / g_material2 and g_mask receives a contiguous fp32 gradient with one value
 * per OUTPUT pixel and material ([B][3|1][H][W]; g_mask [B][1][H][W]); a map or mask that the batch shares (batch_stride 0) owns
 * the sum over the batch, which is left to the caller (pbr_fold_gradient).
 * TILED maps (ABI 8; desc.map_height / map_width: MaterialBase.tile of the blended material, base.py:524-537 -- the blend itself is
 * map-sized, examples/example_blend.py:14-16): every gradient is MAP-sized ([B][3|1][map_height][map_width]; g_mask likewise), each texel
 * owning the sum over its repeats: one kernel blends once per texel, visits the repeats (the walk of pbr_cook_torrance_backward_folded) and
 * runs the folded gradients through the blend's chain rule.  One light, fp32, map widths of whole 4-texel groups, whole outputs or row bands
 * that hold a period of the map's rows: pbr_blend_backward_serves(desc) says whether a descriptor is served (1) or the call would return
 * PBR_ERR_UNSUPPORTED (0: evaluate the differentiable pieces -- pbr_blend_maps_backward, pbr_decode_normal_backward, the folded backward).
 */
int pbr_blend_backward_serves(const pbr_render_desc *desc);
typedef struct pbr_map_grads { void *albedo, *normal, *roughness, *metallic, *specular; } pbr_map_grads;
int pbr_cook_torrance_blend_backward(const pbr_render_desc *desc, const pbr_blend_desc *blend, void *workspace, const void *grad_out,
                                     const pbr_map_grads *g_material1, const pbr_map_grads *g_material2, void *g_mask, void *stream);

/*
 * Gradient of pbr_cook_torrance w.r.t. the maps (what torch.autograd computes through
 * cooktorrance.py:92-182 in the reference's rendering-loss use,
 * docs/source/tutorials/06_advanced.rst:73-107).  `desc` is the forward descriptor (its `out` is
 * ignored; out_dtype must be PBR_F32), fp32 or fp16 maps, any workflow (CONVERTED: gradients w.r.t. the
 * metallic-workflow maps, through the in-kernel conversion); `grad_out` is [B][3][H][W] fp32 contiguous.
 * Each non-NULL g_* receives a contiguous gradient in the maps' storage type, shaped like its map
 * ([B][3|1][H][W]); NULL skips it.  Same sub-gradient conventions as torch (clamp passes on the
 * closed interval).  With tiled maps (map_height/map_width) the g_* are OUTPUT-sized: one value per
 * output pixel; the gradient of a texel is the sum over its repeats -- pbr_cook_torrance_backward_folded hands that out directly.
 * fp16 maps with one light, rows of a whole number of 128 pixels and 4-byte-aligned planes take a streamed kernel (persistent
 * waves, the next tile prefetched global -> LDS); every other launch the one-tile kernels -- same values either way.
 */
int pbr_cook_torrance_backward(const pbr_render_desc *desc, const void *grad_out, void *g_albedo,
                               void *g_normal, void *g_roughness, void *g_metallic, void *g_specular,
                               void *stream);

/*
 * Gradient w.r.t. TILED maps, folded: MaterialBase.tile (base.py:524-537) is map.repeat(1, n, n), so autograd gives a texel the SUM of
 * the gradients of its repeats (the reference's example material is resize(512).tile(2), examples/example_brdf.py:11; its documented
 * ML use a rendering loss over such a material, docs/source/tutorials/06_advanced.rst:73-107).  Arguments as pbr_cook_torrance_backward,
 * but every non-NULL g_* is shaped like its MAP -- [B][3|1][map_height][map_width], contiguous, the maps' storage type -- and receives
 * the sum over the map's repeats inside the output the descriptor describes (the whole tiled image, or a row band of it that holds
 * at least one full period of the map's rows: a multi-GPU shard, whose partial sums the caller adds up across ranks).
 * Map rows a whole number of 4-texel groups (one or several lights): ONE kernel walks the maps, re-evaluates each texel's
 * light-independent terms once, visits its repeats and accumulates in registers (12 B per output pixel + 64 B per texel; under ONE
 * directional light, whose repeats all evaluate alike, the upstream values are summed first and the texel is differentiated once);
 * `workspace` may be NULL.  Other launches (ragged map widths) run pbr_cook_torrance_backward into `workspace`
 * (pbr_backward_folded_workspace_bytes(desc) bytes of device memory, 0 when the one-kernel form serves the descriptor) followed by
 * pbr_fold_gradient_typed per map: the same values to fp32 rounding (the one-kernel form sums a texel's adjoints over its repeats and
 * applies the light-independent tail of the chain rule once; the two-kernel form adds up per-repeat gradients); fp16 gradients are
 * rounded once instead of per repeat.
 * Untiled descriptors are passed on to pbr_cook_torrance_backward.
 */
size_t pbr_backward_folded_workspace_bytes(const pbr_render_desc *desc);
int pbr_cook_torrance_backward_folded(const pbr_render_desc *desc, const void *grad_out, void *g_albedo, void *g_normal,
                                      void *g_roughness, void *g_metallic, void *g_specular, void *workspace, void *stream);

/*
 * The same, plus the gradient w.r.t. the view / light parameters: the reference's forward is plain torch ops on
 * view_dir, light_dir_or_position and light_intensity (cooktorrance.py:95-96, :126-140), so its autograd reaches them
 * (e.g. optimising a light position against a photograph).  `g_params`: (3 + 6 L) floats of DEVICE memory, written as
 * [d/d view_dir (3) | d/d lights (L x 3) | d/d intensities (L x 3)] -- w.r.t. the values in the descriptor (view and
 * directional lights un-normalised: the F.normalize Jacobian of :95 / :126 is applied); light_size is a Python float
 * upstream and has no gradient.  `workspace`: pbr_param_grad_workspace_bytes(desc) bytes of device memory (per-workgroup
 * partial sums, added up in fp64 in a fixed order by a second small kernel on `stream`: deterministic).  Any of the
 * map gradients may be NULL.
 */
size_t pbr_param_grad_workspace_bytes(const pbr_render_desc *desc);
int pbr_cook_torrance_backward_params(const pbr_render_desc *desc, const void *grad_out, void *g_albedo,
                                      void *g_normal, void *g_roughness, void *g_metallic, void *g_specular,
                                      void *g_params, void *workspace, void *stream);

/*
 * The rendering-loss step of docs/source/tutorials/06_advanced.rst:73-107 for the PREDICTED material, as one pass:
 *     loss = nn.MSELoss()(CookTorranceBRDF(...)(predicted_material, ...), target);  loss.backward()
 * `desc` describes the predicted material and the evaluation exactly as for pbr_cook_torrance (its `out` is ignored; out_dtype
 * PBR_F32; fp32 or fp16 maps; any workflow, light type and light count); `target` is the reference rendering
 * [B][3][H][W] fp32 contiguous (e.g. pbr_cook_torrance of the ground-truth material, computed once).  Writes *loss (a DEVICE
 * float) = mean((out - target)^2) over all B*3*H*W values and, into every non-NULL g_*, d loss / d map -- contiguous, shaped
 * like the map, in the maps' storage type -- with torch's sub-gradient conventions, as pbr_cook_torrance_backward.  The
 * colour is never written: 32 + 12 bytes read and 32 written per pixel, against 44 + 36 + 76 for evaluate / MSE / backward.
 * `workspace`: pbr_mse_step_workspace_bytes(desc) bytes of device memory (one partial sum per workgroup, added in fp64 in a
 * fixed order by a second small kernel on `stream`: deterministic).  An upstream gradient other than 1 (loss * k) is applied
 * afterwards with pbr_scale_by_device_scalar, which returns at once when the scalar is 1.
 * Tiled maps (map_height / map_width, the whole output): the g_* are MAP-sized and receive the sum over the repeats, as from
 * pbr_cook_torrance_backward_folded, out of one pass over the maps and the target (12 B per output pixel + 64 B per texel); served
 * for one light and map rows of a whole number of 4-texel groups, PBR_ERR_UNSUPPORTED otherwise (pbr_mse_step_workspace_bytes
 * returns 0 then): the caller evaluates, compares and calls pbr_cook_torrance_backward_folded.
 */
size_t pbr_mse_step_workspace_bytes(const pbr_render_desc *desc);
int pbr_cook_torrance_mse_step(const pbr_render_desc *desc, const void *target, void *g_albedo, void *g_normal, void *g_roughness,
                               void *g_metallic, void *g_specular, void *loss, void *workspace, void *stream);
/*
 * A light stack (an extension: upstream has no counterpart beyond the tutorial's loss applied to L photographs): the L lights of `desc`
 * -- 1 <= L <= PBR_MAX_LIGHTS, one light type, one view direction, one light_size -- are L IMAGES, not one summed image.  Image l is exactly
 * what pbr_cook_torrance gives for light l alone (its own clamp, its own encode).  `desc` as for pbr_cook_torrance, but `desc->out` receives
 * [B][L][3][height][width] fp32, contiguous.  The maps are read and decoded once, the light-independent terms formed once per pixel.
 * Untiled maps (fp32 or fp16, all workflows, both light types, device_params), out_dtype PBR_F32 (else PBR_ERR_DTYPE), both out strides 0:
 * anything else returns PBR_ERR_UNSUPPORTED before any launch.
 */
int pbr_cook_torrance_stack(const pbr_render_desc *desc, void *stream);
/*
 * The rendering-loss step over a light stack, as one pass: loss = nn.MSELoss()(stack(predicted material), targets) and its backward, a
 * capture being L photographs from one camera position with the light moved between the shots.  `targets` is [B][L][3][H][W] fp32
 * contiguous; *loss (a DEVICE float) = the mean over all 3 B L H W values; every non-NULL g_* receives the gradient SUMMED over the lights,
 * contiguous, shaped like the map, in the maps' storage type, with torch's sub-gradient conventions as pbr_cook_torrance_mse_step applies
 * them.  Maps read once, targets once, gradients written once: 64 + 12 L bytes per pixel (fp32) against 76 L + 96 (L - 1) for L steps
 * and autograd's accumulation.  `workspace`: the block pbr_mse_step_workspace_bytes(desc) describes (one partial sum per workgroup, then the
 * stage sums; finished in fp64 in a fixed order: deterministic).  `desc->out` is ignored.  Tiled maps: PBR_ERR_UNSUPPORTED (there is no
 * streamed, tiled or blended form); a NULL targets / loss / workspace: PBR_ERR_NULL_MAP.  No gradients of the lights from this form.
 * (They come from pbr_cook_torrance_mse_stack_fit_step, below.)
 */
int pbr_cook_torrance_mse_stack_step(const pbr_render_desc *desc, const void *targets, void *g_albedo, void *g_normal, void *g_roughness,
                                     void *g_metallic, void *g_specular, void *loss, void *workspace, void *stream);
/*
 * The same step with the gradients of the lights and the view, for captures whose light positions, per-shot intensities or camera axis are
 * fitted along with (or instead of) the maps: everything pbr_cook_torrance_mse_stack_step does, plus `g_params` -- (3 + 6 L) floats of DEVICE
 * memory in pbr_cook_torrance_backward_params's order and meaning: [d/d view_dir (3) | d/d lights (L x 3) | d/d intensities (L x 3)] of the
 * mean over all 3 B L H W values, w.r.t. the values in the descriptor or the device_params block (view and directional lights un-normalised:
 * the F.normalize Jacobian is applied); light_size has no gradient.  Still one pass over the maps; the per-workgroup rows are added up in fp64
 * in a fixed order (deterministic).  Any or all of the g_* maps may be NULL (only the lights are fitted).  `workspace`:
 * pbr_mse_stack_fit_workspace_bytes(desc) bytes of device memory -- the loss partials and stage sums as pbr_mse_step_workspace_bytes lays them
 * out, then one row of 3 + 6 L floats per workgroup (8-byte aligned), then their stage sums; 0 where the call does not serve the descriptor.
 * Before any launch: a NULL g_params / targets / loss / workspace PBR_ERR_NULL_MAP; out_dtype not PBR_F32 PBR_ERR_DTYPE; tiled maps or a NaN
 * light_size PBR_ERR_UNSUPPORTED; more workgroups than the size query promised PBR_ERR_SHAPE.
 */
size_t pbr_mse_stack_fit_workspace_bytes(const pbr_render_desc *desc);
int pbr_cook_torrance_mse_stack_fit_step(const pbr_render_desc *desc, const void *targets, void *g_albedo, void *g_normal, void *g_roughness,
                                         void *g_metallic, void *g_specular, void *g_params, void *loss, void *workspace, void *stream);
/*
 * The perspective camera (an extension: upstream's view_dir is one direction for the whole image, i.e. an orthographic camera).  `desc` as for
 * pbr_cook_torrance, but `desc->view_dir` is a camera POSITION C in the coordinates of a point light's position: the surface point of pixel
 * (y, x) is P = (xs[x], -ys[y], 0) with xs = linspace(-s/2, s/2, width), ys = linspace(-s/2, s/2, height_total), s = light_size or 1.0
 * (cooktorrance.py:130-136; the same grid for both light types), and that pixel's view vector is F.normalize(C - P).  Pixel (y, x) of the result
 * equals pixel (y, x) of upstream's forward called with view_dir = C - P(y, x); a camera exactly on a pixel gives the zero view vector there,
 * as F.normalize does.  fp32 or fp16 maps, all workflows, both light types, 1..PBR_MAX_LIGHTS lights summed as pbr_cook_torrance sums them,
 * batches, row bands (y_offset / height_total), both out strides; with device_params the position is the block's un-normalised view (the
 * `view_dir` handed to pbr_prepare_device_params), lights and intensities the block's.  Before any launch: tiled maps (map_height / map_width)
 * PBR_ERR_UNSUPPORTED; out_dtype not PBR_F32 PBR_ERR_DTYPE; the codes of pbr_cook_torrance for everything else.  A NaN light_size fills the
 * result with NaN for either light type (the grid is NaN).
 */
int pbr_cook_torrance_camera(const pbr_render_desc *desc, void *stream);
/*
 * Its gradient: arguments as pbr_cook_torrance_backward_params (grad_out [B][3][H][W] fp32 contiguous; every non-NULL g_* contiguous, shaped
 * like its map, in the maps' storage type; any may be NULL), and `g_params` may be NULL too: (3 + 6 L) floats of DEVICE memory, written as
 * [d/d camera position (3) | d/d lights (L x 3) | d/d intensities (L x 3)] w.r.t. the values in the descriptor or the device_params block.  The
 * camera's gradient is the sum over pixels of (I - v v^T) / |C - P| g_v, the normalisation Jacobian applied per pixel before the sum;
 * directional lights keep theirs behind it, as in pbr_cook_torrance_backward_params.  `workspace`: pbr_camera_backward_workspace_bytes(desc)
 * bytes of device memory (one row of partial sums per workgroup, then their stage sums: added up in fp64 in a fixed order, deterministic; 0
 * where the call does not serve the descriptor); only read or written when g_params is given.  Before any launch: the codes of
 * pbr_cook_torrance_camera; a NULL grad_out, or a g_params without a workspace, PBR_ERR_NULL_MAP; a NaN light_size PBR_ERR_UNSUPPORTED; more
 * workgroups than the size query promised PBR_ERR_SHAPE.
 */
size_t pbr_camera_backward_workspace_bytes(const pbr_render_desc *desc);
int pbr_cook_torrance_camera_backward(const pbr_render_desc *desc, const void *grad_out, void *g_albedo, void *g_normal, void *g_roughness,
                                      void *g_metallic, void *g_specular, void *g_params, void *workspace, void *stream);
/*
 * Light stacks under the perspective camera: pbr_cook_torrance_stack, pbr_cook_torrance_mse_stack_step and
 * pbr_cook_torrance_mse_stack_fit_step with `desc->view_dir` a camera POSITION, as for pbr_cook_torrance_camera.  Image l of the stack is what
 * pbr_cook_torrance_camera gives for light l alone (its own clamp, its own encode); the stack and `targets` are [B][L][3][H][W] fp32
 * contiguous; *loss, the g_* and the workspaces are the orthographic steps'; `g_params` is [d/d camera position (3) | d/d lights (L x 3) |
 * d/d intensities (L x 3)], the position's gradient as pbr_cook_torrance_camera_backward forms it.  fp32 or fp16 maps, all workflows, both
 * light types, batches; with device_params the position is the block's un-normalised view, read at every launch.  One pass over the maps,
 * deterministic.  Workspaces: pbr_mse_step_workspace_bytes(desc) for the step, pbr_camera_mse_stack_fit_workspace_bytes(desc) for the fit step
 * (the layout and size of pbr_mse_stack_fit_workspace_bytes; 0 where the call does not serve the descriptor).
 * Before any launch -- the stack: the codes of pbr_cook_torrance_camera (map_height / map_width set at all PBR_ERR_UNSUPPORTED, an fp16 result
 * PBR_ERR_DTYPE), out strides PBR_ERR_UNSUPPORTED; a NaN light_size fills the whole stack with NaN.  The steps: a NULL targets / loss /
 * workspace (fit: / g_params) PBR_ERR_NULL_MAP; out_dtype not PBR_F32 PBR_ERR_DTYPE; map_height / map_width set at all, or a NaN light_size
 * (either light type), PBR_ERR_UNSUPPORTED; more workgroups than the size query promised PBR_ERR_SHAPE.
 */
int pbr_cook_torrance_camera_stack(const pbr_render_desc *desc, void *stream);
int pbr_cook_torrance_camera_mse_stack_step(const pbr_render_desc *desc, const void *targets, void *g_albedo, void *g_normal, void *g_roughness,
                                            void *g_metallic, void *g_specular, void *loss, void *workspace, void *stream);
size_t pbr_camera_mse_stack_fit_workspace_bytes(const pbr_render_desc *desc);
int pbr_cook_torrance_camera_mse_stack_fit_step(const pbr_render_desc *desc, const void *targets, void *g_albedo, void *g_normal, void *g_roughness,
                                                void *g_metallic, void *g_specular, void *g_params, void *loss, void *workspace, void *stream);
/*
 * Light stacks with one camera position PER SHOT (a handheld capture: the camera moves with the flash): the three camera-stack calls with the
 * L positions handed over beside the descriptor -- `desc->view_dir` and the device_params block's view are not read.  Image l of the stack is
 * what pbr_cook_torrance_camera gives for position l and light l alone: its own view vectors F.normalize(C_l - P(y, x)), its own clamp, its own
 * encode.  Exactly one of `cameras_host` / `cameras_device` is non-NULL: `cameras_host` is float[L][3] in host memory, read now (the values
 * travel in the kernel arguments); `cameras_device` is float[L][3] fp32 in DEVICE memory, read by the kernel when it runs -- no read-back,
 * nothing baked in, so a captured graph sees the positions' current values at every replay.  Lights and intensities: the descriptor or its
 * device_params block, as everywhere.  Stack, `targets`, *loss, the g_* and the step's workspace are the camera stack's; `g_params` is 9 L
 * floats of DEVICE memory, [d/d cameras (L x 3) | d/d lights (L x 3) | d/d intensities (L x 3)]: each position's gradient the sum over pixels
 * of (I - v v^T) / |C_l - P| g_v, applied per pixel before the sum; directional lights behind their F.normalize Jacobian.  The fit step's
 * workspace is pbr_view_mse_stack_fit_workspace_bytes(desc): the camera fit layout with rows of 9 L floats (0 where the call does not serve
 * the descriptor).  64 + 12 L bytes per pixel like the other stacks; one pass over the maps, deterministic.
 * Before any launch: the codes of the camera-stack calls, and both or neither of the two camera pointers PBR_ERR_NULL_MAP.
 */
int pbr_cook_torrance_view_stack(const pbr_render_desc *desc, const float *cameras_host, const void *cameras_device, void *stream);
int pbr_cook_torrance_view_mse_stack_step(const pbr_render_desc *desc, const float *cameras_host, const void *cameras_device, const void *targets,
                                          void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic, void *g_specular, void *loss,
                                          void *workspace, void *stream);
size_t pbr_view_mse_stack_fit_workspace_bytes(const pbr_render_desc *desc);
int pbr_cook_torrance_view_mse_stack_fit_step(const pbr_render_desc *desc, const float *cameras_host, const void *cameras_device, const void *targets,
                                              void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic, void *g_specular,
                                              void *g_params, void *loss, void *workspace, void *stream);
/*
 * The six stack loss steps with a weight per pixel -- a capture with a mask: coverage that differs from shot to shot, clipped highlights,
 * confidence.  *loss = mean over all 3 B L H W elements of w (image - target)^2, the weight the same for the three channels; N stays 3 B L H W,
 * the sum of the weights is not used (a caller who wants the mean over valid pixels divides by the constant mean of the weights).  Every g_*
 * and g_params is the gradient of that loss.  `weights` is fp32 DEVICE memory, never NULL; the weight of pixel (y, x) of shot l of material b is
 * weights[b * w_batch_stride + l * w_light_stride + y * W + x], the strides in elements, the address formed in 64-bit arithmetic.
 * `w_light_stride` is H W (a plane per shot) or 0 (one plane for all shots); `w_batch_stride` is the caller's (L H W or H W for dense weights).
 * Everything else -- `targets`, the g_*, `g_params` and its layout, *loss, the camera pointers of the view calls -- is the unweighted call's,
 * and so are the workspaces: pbr_mse_step_workspace_bytes for the steps, pbr_mse_stack_fit_workspace_bytes /
 * pbr_camera_mse_stack_fit_workspace_bytes / pbr_view_mse_stack_fit_workspace_bytes for the fit steps; the weights add no workspace.
 * Bytes per pixel (fp32 maps, metallic workflow): 64 + 16 L with a plane per shot, 68 + 12 L with one plane.  One pass, deterministic.
 * No sign check: a negative weight is the caller's business.  A weight of exactly 0 beside a finite target and a finite render contributes
 * exactly +-0 to the loss and to every gradient; a NaN target under a zero weight still gives NaN (0 * NaN).
 * Before any launch: the codes of the unweighted call, NULL `weights` PBR_ERR_NULL_MAP like the other pointers, then a `w_light_stride` that is
 * neither 0 nor H W PBR_ERR_SHAPE.
 */
int pbr_cook_torrance_weighted_mse_stack_step(const pbr_render_desc *desc, const void *targets, const void *weights, int64_t w_batch_stride,
                                              int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                              void *g_specular, void *loss, void *workspace, void *stream);
int pbr_cook_torrance_weighted_mse_stack_fit_step(const pbr_render_desc *desc, const void *targets, const void *weights, int64_t w_batch_stride,
                                                  int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                                  void *g_specular, void *g_params, void *loss, void *workspace, void *stream);
int pbr_cook_torrance_camera_weighted_mse_stack_step(const pbr_render_desc *desc, const void *targets, const void *weights, int64_t w_batch_stride,
                                                     int64_t w_light_stride, void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic,
                                                     void *g_specular, void *loss, void *workspace, void *stream);
int pbr_cook_torrance_camera_weighted_mse_stack_fit_step(const pbr_render_desc *desc, const void *targets, const void *weights,
                                                         int64_t w_batch_stride, int64_t w_light_stride, void *g_albedo, void *g_normal,
                                                         void *g_roughness, void *g_metallic, void *g_specular, void *g_params, void *loss,
                                                         void *workspace, void *stream);
int pbr_cook_torrance_view_weighted_mse_stack_step(const pbr_render_desc *desc, const float *cameras_host, const void *cameras_device,
                                                   const void *targets, const void *weights, int64_t w_batch_stride, int64_t w_light_stride,
                                                   void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic, void *g_specular,
                                                   void *loss, void *workspace, void *stream);
int pbr_cook_torrance_view_weighted_mse_stack_fit_step(const pbr_render_desc *desc, const float *cameras_host, const void *cameras_device,
                                                       const void *targets, const void *weights, int64_t w_batch_stride, int64_t w_light_stride,
                                                       void *g_albedo, void *g_normal, void *g_roughness, void *g_metallic, void *g_specular,
                                                       void *g_params, void *loss, void *workspace, void *stream);
/* ABI 5: view / light / intensity from DEVICE memory.  `view_dir` [3], `lights` [n_lights][3], `intensities` [intensity_rows][3] with
 * intensity_rows = 1 (one intensity for every light) or n_lights: fp32 device pointers; a NULL pointer takes that parameter from the descriptor
 * (d->view_dir / d->lights / d->intensities: host values), so only what lives on the device needs to be there.  Writes `block` (pbr_device_params_bytes() bytes,
 * 16-byte aligned): the normalised view vector and per light what pbr_cook_torrance otherwise folds on the host (cooktorrance.py:95-96,
 * :126-127, :155-158).  Reads d->light_type, d->n_lights and the host parameters of the descriptor.  Put the block's address into pbr_render_desc.device_params of the
 * launches that follow on the stream (forward, backward, backward_params, blend, mse_step). */
size_t pbr_device_params_bytes(void);
int pbr_prepare_device_params(const pbr_render_desc *d, const void *view_dir, const void *lights, const void *intensities,
                              int32_t intensity_rows, void *block, void *stream);

/* data[i] *= *scalar for n elements of `dtype`, in place; `scalar` is a DEVICE float (no host synchronisation: the upstream
 * gradient of a loss lives on the device); a scalar of exactly 1 leaves the data untouched. */
int pbr_scale_by_device_scalar(void *data, size_t n, int dtype, const void *scalar, void *stream);
/* The same for up to five buffers of one dtype in ONE launch (the gradients a step leaves): data[j] has n[j] elements, count <= 5. */
int pbr_scale_list_by_device_scalar(void *const *data, const size_t *n, int count, int dtype, const void *scalar, void *stream);

/* ---- stand-alone map conversions (same arithmetic as the fused kernel) ------------- */

/* utils.srgb_to_linear, pypbr/utils/functions.py:31-47.  n elements, in-place allowed. */
int pbr_srgb_to_linear(const void *src, void *dst, size_t n, int dtype, void *stream);
/* utils.linear_to_srgb, pypbr/utils/functions.py:50-66. */
int pbr_linear_to_srgb(const void *src, void *dst, size_t n, int dtype, void *stream);

/*
 * BasecolorMetallicMaterial.to_diffuse_specular_material, metallic.py:98-108:
 * diffuse = a(1-m), specular = 0.04(1-m) + a m on LINEAR albedo (decoded here when
 * albedo_is_srgb).  albedo [B][3][P], metallic [B][1][P] -> diffuse, specular [B][3][P].
 */
int pbr_metallic_to_specular(const void *albedo, const void *metallic, void *diffuse, void *specular,
                             int32_t batch, int64_t pixels, int albedo_is_srgb, int dtype, void *stream);
/*
 * DiffuseSpecularMaterial.to_basecolor_metallic_material, diffuse.py:128-147 (raw
 * specular, 3-channel metallic).  diffuse, specular [n] -> basecolor, metallic [n].
 */
int pbr_specular_to_metallic(const void *diffuse, const void *specular, void *basecolor, void *metallic,
                             size_t n, int albedo_is_srgb, int dtype, void *stream);
/*
 * Gradients of the four conversions above w.r.t. their inputs -- what torch.autograd derives from the reference's plain torch
 * ops, so that a rendering loss differentiates through material.to_linear() / to_srgb() (base.py:754-778), the lazy
 * linear_albedo / linear_specular properties (base.py:262-277, diffuse.py:76-91), to_diffuse_specular_material (metallic.py:98-108)
 * and to_basecolor_metallic_material (diffuse.py:128-147) exactly as upstream.  torch's sub-gradient conventions: clamp passes on
 * the closed interval; masked assignment / torch.where route the gradient to the selected branch; the thresholded selects of
 * diffuse.py:136-144 are re-taken with the forward's own arithmetic.  `src` / the maps are the FORWARD INPUTS; gradients have the
 * maps' storage type and shape.  An upstream gradient that is NULL counts as zero (that output was not used); a result pointer
 * that is NULL is not computed.
 */
int pbr_srgb_to_linear_backward(const void *src, const void *grad_out, void *grad_in, size_t n, int dtype, void *stream);
int pbr_linear_to_srgb_backward(const void *src, const void *grad_out, void *grad_in, size_t n, int dtype, void *stream);
int pbr_metallic_to_specular_backward(const void *albedo, const void *metallic, const void *g_diffuse, const void *g_specular,
                                      void *g_albedo, void *g_metallic, int32_t batch, int64_t pixels, int albedo_is_srgb, int dtype,
                                      void *stream);
int pbr_specular_to_metallic_backward(const void *diffuse, const void *specular, const void *g_basecolor, const void *g_metallic,
                                      void *g_diffuse, void *g_specular, size_t n, int albedo_is_srgb, int dtype, void *stream);

/* Gradient of pbr_decode_normal w.r.t. the stored map (what autograd computes through base.py:191-242 when a predicted
 * normal map is assigned to a material in a rendering loss): fp32, `workspace` = the flag pbr_decode_normal left. */
int pbr_decode_normal_backward(const void *src, const void *grad_out, void *grad_in, int32_t channels, int64_t pixels,
                               const void *workspace, void *stream);

/* Gradient folding behind pbr_cook_torrance_backward (the sums torch.autograd would perform for a broadcast or a
 * repeat(): a map shared by the whole batch, or tiled ny x nx by map_height/map_width, owns the sum of the
 * per-output-pixel gradients).  src [batch][channels][ny*h][nx*w] fp32 contiguous ->
 * dst [fold_batch ? 1 : batch][channels][h][w]. */
int pbr_fold_gradient(const void *src, void *dst, int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t ny,
                      int32_t nx, int fold_batch, void *stream);
/* The same for gradients stored as the maps are (pbr_cook_torrance_backward returns fp16 gradients for fp16 maps): `dtype`
 * PBR_F32 | PBR_F16 for src and dst alike, the sums are formed in fp32 and rounded once. */
int pbr_fold_gradient_typed(const void *src, void *dst, int32_t batch, int32_t channels, int32_t h, int32_t w, int32_t ny,
                            int32_t nx, int fold_batch, int dtype, void *stream);

/*
 * MaterialBase._process_normal_map, base.py:191-242.  channels = 2 or 3, planar
 * [channels][pixels] -> [3][pixels].  3 channels: kept as-is when any value is
 * negative, else x*2-1 and unit length.  `workspace` = 4 bytes of device memory
 * (the min<0 flag; written by the call: 1 when the map was kept as it is).
 * Source and destination disjoint: the map is read once (twice when it is kept
 * as it is only because of a negative value the 4096-sample probe missed).
 * `dst == src` is allowed: flag pass first, then the transform.
 */
int pbr_decode_normal(const void *src, void *dst, int32_t channels, int64_t pixels, int dtype,
                      void *workspace, void *stream);

/*
 * The normal-map operations of pypbr/utils/functions.py:69-177 and pypbr/materials/base.py:673-729 on the device.  Height
 * [batch][1][height][width], normals [batch][3][height][width]; rows dense, strides in ELEMENTS (batch_stride between images,
 * plane_stride between the x / y / z planes), any non-negative values.  Forwards: `dtype` PBR_F32 | PBR_F16 storage, fp32 arithmetic
 * in the reference's rounding order (IEEE sqrt and division).  Backwards: fp32.  No workspace; a bad shape, stride or dtype returns
 * PBR_ERR_SHAPE / PBR_ERR_DTYPE before anything is launched.
 *
 * pbr_normal_from_height: utils.compute_normal_from_height, functions.py:123-177 (and MaterialBase.compute_normal_from_height,
 * base.py:708-729).  Zero padding at every image's border (the images of a batch never see each other):
 *   gx = h(y,x-1) - h(y,x+1), gy = h(y-1,x) - h(y+1,x), a = -(gx scale), b = -(gy scale) (OpenGL, directx 0) | +(gy scale) (DirectX),
 *   n = (a, b, 1) / |(a, b, 1)|.  No clamps: a NaN height gives NaN exactly where the reference's does.
 */
int pbr_normal_from_height(const void *height, int64_t height_batch_stride, void *normal, int64_t normal_batch_stride,
                           int64_t normal_plane_stride, int32_t batch, int32_t height_px, int32_t width, float scale, int32_t directx,
                           int dtype, void *stream);
/* Gradient of pbr_normal_from_height w.r.t. the height (what autograd derives from functions.py:146-175): g_v = (g_n - n (n . g_n)) / |v|
 * per pixel, then the transposed stencil of (g_a, g_b).  fp32; `height` is the forward's input. */
int pbr_normal_from_height_backward(const void *height, int64_t height_batch_stride, const void *grad_normal, int64_t grad_batch_stride,
                                    int64_t grad_plane_stride, void *grad_height, int64_t grad_height_batch_stride, int32_t batch,
                                    int32_t height_px, int32_t width, float scale, int32_t directx, void *stream);
/*
 * The per-pixel transforms: (x, y) <- M (x, y) with M = [[m00, m01], [m10, m11]], z kept, then, when `renormalize`, F.normalize
 * (v / max(|v|, 1e-12)).  `pixels` = height * width per image; `dst == src` is allowed (the in-place utilities).
 *   utils.rotate_normals, functions.py:69-108:                    M = R(angle), renormalised
 *   utils.invert_normal, functions.py:111-120 (base.py:673-687): M = diag(1, -1), not renormalised (an exact negation)
 *   MaterialBase.adjust_normal_strength, base.py:689-706:         M = f I, renormalised
 * A diagonal M scales x and y by one multiplication each, as the reference's in-place products do.
 */
int pbr_normal_transform(const void *src, int64_t src_batch_stride, int64_t src_plane_stride, void *dst, int64_t dst_batch_stride,
                         int64_t dst_plane_stride, int32_t batch, int64_t pixels, float m00, float m01, float m10, float m11,
                         int32_t renormalize, int dtype, void *stream);
/* Gradient of pbr_normal_transform w.r.t. its source: g_v = renormalize ? (g - n (n . g)) / |v| : g, g_xy = M^T g_v_xy, g_z = g_v_z.
 * fp32; `src` is the forward's input (not its result). */
int pbr_normal_transform_backward(const void *src, int64_t src_batch_stride, int64_t src_plane_stride, const void *grad_out,
                                  int64_t grad_batch_stride, int64_t grad_plane_stride, void *grad_in, int64_t grad_in_batch_stride,
                                  int64_t grad_in_plane_stride, int32_t batch, int64_t pixels, float m00, float m01, float m10, float m11,
                                  int32_t renormalize, void *stream);

/*
 * Normal -> height by Poisson reconstruction: utils.compute_height_from_normal, pypbr/utils/functions.py:180-323 (and
 * MaterialBase.compute_height_from_normal, base.py:731-751), everything but the two Fourier transforms.  The caller
 * runs, per batch:   pbr_normal_divergence -> rfft2 -> pbr_poisson_scale -> irfft2(s = (H, W)) -> pbr_height_stats -> pbr_height_normalize
 * and, backwards:    pbr_height_normalize_backward -> rfft2 -> pbr_poisson_scale -> irfft2 -> pbr_normal_divergence_backward
 * (the solve is its own adjoint: its denominators are real and even).  Normals [batch][3][height][width], every other map
 * [batch][height][width]; rows dense, strides in ELEMENTS, any non-negative values; height * width < 2^31.  `dtype` PBR_F32 | PBR_F16 is
 * the storage of the normals (divergence) and of the height map (normalize); everything in between and every backward is fp32.  A bad
 * shape, stride, alignment or dtype returns PBR_ERR_SHAPE / PBR_ERR_DTYPE before anything is launched.  The images of a batch never
 * see each other; no kernel uses atomics, and the same input gives the same bits on every run.
 *
 * pbr_normal_divergence: functions.py:205-228, :250-283, bit-equal to upstream's div_g.  ze = n_z + 1e-8, g_x = (-n_x / ze) scale,
 *   g_y = (-n_y / ze) scale (OpenGL, directx 0) | (+n_y / ze) scale (DirectX);  div = (g_x(y,x+1) - g_x(y,x)) + (g_y(y+1,x) - g_y(y,x)),
 *   the last column's x difference and the last row's y difference being g - g (replicate padding).  No clamps.  `div` is fp32.
 */
int pbr_normal_divergence(const void *normal, int64_t normal_batch_stride, int64_t normal_plane_stride, void *div, int64_t div_batch_stride,
                          int32_t batch, int32_t height_px, int32_t width, float scale, int32_t directx, int dtype, void *stream);
/* Gradient of pbr_normal_divergence w.r.t. the normals, a gather: a_x(y,x) = dd(y,x-1) [x >= 1] - dd(y,x) [x <= W-2], a_y likewise along y;
 * g_nx = -scale a_x / ze, g_ny = -+scale a_y / ze, g_nz = scale (n_x a_x +- n_y a_y) / ze^2 (upper signs: OpenGL).  fp32; `normal` is the
 * forward's input. */
int pbr_normal_divergence_backward(const void *normal, int64_t normal_batch_stride, int64_t normal_plane_stride, const void *grad_div,
                                   int64_t grad_div_batch_stride, void *grad_normal, int64_t grad_batch_stride, int64_t grad_plane_stride,
                                   int32_t batch, int32_t height_px, int32_t width, float scale, int32_t directx, void *stream);
/* functions.py:286-323 between its transforms, in place on the half spectrum [batch][height_px][width / 2 + 1] of interleaved complex64
 * (8-byte aligned; `spectrum_batch_stride` in complex elements; `width` is the REAL width): both components divided by
 * den(ky, kx) = -4 (sin^2(pi kx / width) + sin^2(pi ky / height_px)), the DC bin set to 0.  den is upstream's
 * (2 cos(2 pi kx / W) - 2) + (2 cos(2 pi ky / H) - 2) in the form that does not cancel at low frequencies. */
int pbr_poisson_scale(void *spectrum, int64_t spectrum_batch_stride, int32_t batch, int32_t height_px, int32_t width, void *stream);
/* Bytes of the workspace pbr_height_stats / pbr_height_normalize and pbr_height_normalize_backward need (8-byte aligned; 0: bad shape):
 * one 24-byte partial per 12288 pixels of every image. */
size_t pbr_height_workspace_bytes(int32_t batch, int32_t height_px, int32_t width);
/* Per image of `height` (fp32, the inverse transform's output): sum (fp64), min, max and the linear indices of the first minimum and
 * the first maximum, as per-workgroup partials over fixed pixel ranges in `workspace`. */
int pbr_height_stats(const void *height, int64_t height_batch_stride, void *workspace, int32_t batch, int32_t height_px, int32_t width,
                     void *stream);
/* functions.py:234-242: folds the partials in index order (64 consecutive groups one by one, then the groups: a fixed association), then out = ((h - mean) - mn) / ((mx - mn) + 1e-8) with mn = fl(min h - mean),
 * mx = fl(max h - mean), stored as `dtype`; `stats` [batch][5] fp32 receives {mean, mn, range, argmin, argmax}, the two indices as int32
 * bit patterns (what the backward reads). */
int pbr_height_normalize(const void *height, int64_t height_batch_stride, const void *workspace, void *out, int64_t out_batch_stride,
                         void *stats, int32_t batch, int32_t height_px, int32_t width, int dtype, void *stream);
/* Gradient of pbr_height_normalize w.r.t. its input: with r = range, q = sum(G out) / r, s = sum(G) / r (fp64 partials in `workspace`,
 * folded as the forward's), dh = G / r + [i = argmin] (q - s) - [i = argmax] q.  The gradient of min / max goes to the FIRST index (upstream
 * spreads it over ties); the mean subtraction's adjoint vanishes (sum(dh) = 0).  fp32; `out` and `stats` are the forward's results. */
int pbr_height_normalize_backward(const void *grad_out, int64_t grad_batch_stride, const void *out, int64_t out_batch_stride, const void *stats,
                                  void *workspace, void *grad_height, int64_t grad_height_batch_stride, int32_t batch, int32_t height_px,
                                  int32_t width, void *stream);

/*
 * The geometric material transforms of pypbr/materials/base.py -- crop (:506-522, in-bounds), tile (:524-537), flip_horizontal /
 * flip_vertical (:605-639), roll (:641-655) -- and every chain of them as ONE index map per axis:
 *     src(i) = (offset + step * i) mod N,   i in [0, L),   step = +1 | -1,   0 <= offset < N
 * with N the source extent and L the output extent (L < N a crop, L > N a tile).  src [batch][planes][h_src][w_src] ->
 * dst [batch][planes][h_out][w_out]; rows dense, batch and plane strides in ELEMENTS (src: any non-negative value; dst: positive where
 * there is more than one image / plane).  Bit i of `negate_mask` negates plane i (a flip's sign on a normal map's x or y plane), so
 * planes <= 32.  `dtype` PBR_F32 | PBR_F16: values are copied, negated ones have their sign bit flipped -- nothing is rounded.
 * `dst` must NOT overlap `src` (the kernel reads through __restrict__ pointers; a remap is not an in-place operation).
 * A bad shape, stride, offset, step or dtype returns PBR_ERR_SHAPE / PBR_ERR_DTYPE before anything is launched.  No workspace.
 */
int pbr_remap_planes(const void *src, int64_t src_batch_stride, int64_t src_plane_stride, void *dst, int64_t dst_batch_stride,
                     int64_t dst_plane_stride, int32_t batch, int32_t planes, int32_t h_src, int32_t w_src, int32_t h_out, int32_t w_out,
                     int32_t y_offset, int32_t y_step, int32_t x_offset, int32_t x_step, uint32_t negate_mask, int dtype, void *stream);
/* Gradient of pbr_remap_planes w.r.t. `src`, fp32, as a GATHER: source texel p of an axis sums the grad_out values of its preimages
 * i0 + k N < L, i0 = step (p - offset) mod N, in registers and in a fixed order (rows outer, columns inner, k ascending), applies the
 * plane's sign and writes 0 where a crop left no preimage.  No atomics, no workspace; every element of grad_src is written.
 * grad_out [batch][planes][h_out][w_out] -> grad_src [batch][planes][h_src][w_src], strides as above; they must not overlap. */
int pbr_remap_planes_backward(const void *grad_out, int64_t grad_out_batch_stride, int64_t grad_out_plane_stride, void *grad_src,
                              int64_t grad_src_batch_stride, int64_t grad_src_plane_stride, int32_t batch, int32_t planes, int32_t h_src,
                              int32_t w_src, int32_t h_out, int32_t w_out, int32_t y_offset, int32_t y_step, int32_t x_offset,
                              int32_t x_step, uint32_t negate_mask, void *stream);

/*
 * MaterialBase.rotate, base.py:539-603 -- pad, torchvision's nearest-neighbour rotate(expand=True), centre crop and, for the normal map,
 * utils.rotate_normals -- as ONE index function per output pixel.  The host computes the constants below from
 * (h, w, angle, expand, padding_mode); per output pixel (i, j) the kernel evaluates, in fp32 and in this rounding order,
 *     x = j + x0, y = i + y0 (exact);  gx = rn(rn(x t00) + rn(y t10)), gy = rn(rn(x t01) + rn(y t11))   (no fused multiply-add);
 *     fx = ((gx + 1) Wp - 1) / 2, fy = ((gy + 1) Hp - 1) / 2 (each step rounded);  ix = rint(fx), iy = rint(fy) (halves to even)
 * with Hp x Wp = (h + 2 pad) x (w + 2 pad).  Outside [0, Wp) x [0, Hp) the pixel is 0; otherwise `pad` is subtracted and the pixel is 0
 * outside the h x w map (constant padding) or wraps once into it (circular; pad <= h, w).
 */
typedef struct pbr_rotate_geom {
    int32_t pad;                  /* ceil(sqrt(H^2 + W^2)) - H, on all four sides of the h x w map */
    int32_t circular;             /* 0: constant (zero) padding, 1: circular */
    float x0, y0;                 /* left - ow / 2 + 0.5, top - oh / 2 + 0.5: the centre crop inside torchvision's expanded ow x oh image */
    float t00, t10, t01, t11;     /* the inverse matrix cast to fp32 and divided in fp32 by (0.5 Wp, 0.5 Hp): x row t00 t10, y row t01 t11 */
    float cos_r, sin_r;           /* cos and sin of radians(-angle) in fp32 (the backward maps texel centres to output coordinates) */
} pbr_rotate_geom;
/* src [batch][planes][h_src][w_src] -> dst [batch][planes][h_out][w_out]; rows dense, batch and plane strides in ELEMENTS as for
 * pbr_remap_planes; planes <= 32.  Values are copied bit for bit (`dtype` PBR_F32 | PBR_F16), except, when normal_first_plane >= 0,
 * planes normal_first_plane .. + 2 of every pixel: they are a normal map's (x, y, z) and pass through pbr_normal_transform's arithmetic
 * with M = [[m00, m01], [m10, m11]], renormalised (a filled pixel stays 0).  normal_first_plane = -1: no normal map in the block.
 * `dst` must not overlap `src`.  A bad shape, stride, plane index or geometry (a circular pad beyond the map) returns PBR_ERR_SHAPE
 * before anything is launched.  No workspace.  (ABI 9: entry points added, nothing changed.) */
int pbr_rotate_planes(const void *src, int64_t src_batch_stride, int64_t src_plane_stride, void *dst, int64_t dst_batch_stride,
                      int64_t dst_plane_stride, int32_t batch, int32_t planes, int32_t h_src, int32_t w_src, int32_t h_out, int32_t w_out,
                      const pbr_rotate_geom *geom, int32_t normal_first_plane, float m00, float m01, float m10, float m11, int dtype,
                      void *stream);
/* Gradient of pbr_rotate_planes w.r.t. `src`, fp32, as a GATHER over source texels: every place of the texel in the padded image (one;
 * up to three per axis in circular mode) is mapped to output coordinates, and the 3 x 3 output pixels around it that the FORWARD's index
 * function sends to that place are summed in a fixed order (places ascending, then output row, then column).  The normal triple's three
 * sums then pass ONCE through pbr_normal_transform_backward's arithmetic at the texel's own normal, read from `src` (the forward's
 * input; may be NULL when normal_first_plane is -1).  No atomics, no workspace; every element of grad_src is written. */
int pbr_rotate_planes_backward(const void *grad_out, int64_t grad_out_batch_stride, int64_t grad_out_plane_stride, void *grad_src,
                               int64_t grad_src_batch_stride, int64_t grad_src_plane_stride, const void *src, int64_t src_batch_stride,
                               int64_t src_plane_stride, int32_t batch, int32_t planes, int32_t h_src, int32_t w_src, int32_t h_out,
                               int32_t w_out, const pbr_rotate_geom *geom, int32_t normal_first_plane, float m00, float m01, float m10,
                               float m11, void *stream);

/*
 * Packed material tensors: MaterialBase.from_tensor (base.py:416-487), as_tensor (:319-414) and normal_rgb (:279-291) as ONE launch over
 * a table of at most PBR_MAX_PLANE_OPS plane operations, each over [batch] images of `pixels` elements per plane (strides in ELEMENTS):
 *   PBR_PLANE_AFFINE     one plane:  dst = src * scale + bias.  (1, 0) copies; (0.5, 0.5) is from_tensor's is_normalized, (2, -1) as_tensor's
 *                        (t - 0.5) / 0.5: each is one rounding of an exact product, so the results are the reference's bit for bit.
 *   PBR_PLANE_NORMAL_XY  two planes (src, src + src_plane_stride) -> three (dst + k dst_plane_stride): _compute_normal_map_z_component,
 *                        base.py:223-242, after a = src * scale + bias: v = 2 a - 1, s = x^2 + y^2, z = sqrt(max(1 - s, 1e-6)),
 *                        n = (x, y, z) / max(|(x, y, z)|, 1e-12).  x^2, y^2, their sum and 1 - s are each rounded on their own, sqrt and the
 *                        division are IEEE: z is ill-conditioned near the unit circle and this order is what keeps it within 1e-6 there.
 * `dtype` PBR_F32 | PBR_F16 is the storage type of every source and destination (arithmetic in fp32).  Plane bases need element alignment
 * only.  Nothing a launch writes may overlap anything it reads.  Caller errors, before anything is launched: a NULL table, source or
 * destination PBR_ERR_NULL_MAP; n_ops outside [1, PBR_MAX_PLANE_OPS], batch outside [1, 65535], pixels < 1, a negative stride, written
 * planes / images on top of each other, a misaligned pointer or an overlap PBR_ERR_SHAPE; an unknown kind PBR_ERR_UNSUPPORTED; a dtype
 * PBR_ERR_DTYPE.  No workspace.  (ABI 9: entry points added, nothing changed.)
 */
enum { PBR_PLANE_AFFINE = 0, PBR_PLANE_NORMAL_XY = 1 };
#define PBR_MAX_PLANE_OPS 32
typedef struct pbr_plane_op {
    int32_t kind;                 /* PBR_PLANE_* */
    int32_t reserved;
    const void *src;              /* forward: the source plane(s).  backward: the upstream gradient, NULL = zero */
    int64_t src_batch_stride;
    int64_t src_plane_stride;     /* NORMAL_XY only */
    void *dst;                    /* forward: the destination plane(s).  backward: the gradient w.r.t. the forward's source plane(s) */
    int64_t dst_batch_stride;
    int64_t dst_plane_stride;     /* NORMAL_XY only */
    const void *input;            /* backward of NORMAL_XY: the forward's source (x, y planes); ignored otherwise */
    int64_t input_batch_stride;
    int64_t input_plane_stride;
    float scale;
    float bias;
} pbr_plane_op;
int pbr_plane_ops(const pbr_plane_op *ops, int32_t n_ops, int32_t batch, int64_t pixels, int dtype, void *stream);
/* Gradient of pbr_plane_ops w.r.t. every source plane, as a gather over the same table with `src` / `dst` holding gradients (see the
 * struct): AFFINE g scale; NORMAL_XY F.normalize's adjoint (g - n (n . g)) / |v|, z's dependence on x and y where 1 - s >= 1e-6 (torch's
 * clamp passes the gradient there, the bound included; nothing where it clamped), then x 2 and x scale.  Every element of every `dst`
 * is written exactly once; an operation whose `src` is NULL writes zeros.  fp32 only (`dtype` must be PBR_F32). */
int pbr_plane_ops_backward(const pbr_plane_op *ops, int32_t n_ops, int32_t batch, int64_t pixels, int dtype, void *stream);

/*
 * MaterialBase._to_tensor for PIL images, base.py:143-164, on the device: an image's own samples -- uint8 (`bits` 8; torchvision's
 * to_tensor: (H,W,C) -> float32 (C,H,W) / 255) or uint16 (`bits` 16; base.py:146-152: / 65535.0) -- become the float32 planar map
 * dst [channels][height][width] (dense).  The division is IEEE-exact: every one of the 256 / 65 536 possible samples gives the float
 * the reference's CPU code gives.  `src` is addressed as src[c*stride_c + y*stride_h + x*stride_w] (strides in samples), so the
 * (H,W,C) array PIL hands out travels as it is -- a quarter of the bytes of the float map on the host-to-device copy -- and needs
 * no transposing on the host; channels 1..4.
 * decode_normal != 0: the map is a normal map (channels 2 or 3) and base.py:191-242 `_process_normal_map` follows in the same pass --
 * samples are never negative, so :212's "already signed?" is false by construction and the map is always decoded; dst has 3 planes,
 * bit-identical to pbr_decode_normal of the float map.
 */
int pbr_unpack_image(const void *src, int32_t bits, int32_t channels, int32_t height, int32_t width, int64_t stride_c,
                     int64_t stride_h, int64_t stride_w, float *dst, int32_t decode_normal, void *stream);

/*
 * MaterialBase.to_pil, base.py:793-850, on the device -- the way back of pbr_unpack_image: planar float32 maps become image samples,
 * dense (height, width, channels) uint8 (`bits` 8) or uint16 (`bits` 16) arrays as PIL takes them.  ONE launch for a table of at most
 * PBR_MAX_IMAGE_PACKS maps that share (height, width) -- a material's maps as a rule.  `src` is addressed as
 * src[c*stride_c + y*stride_h + x*stride_w] (strides in ELEMENTS, none negative), so a view with a plane pitch or a row pitch is read as
 * it is.  Arithmetic, every product and sum rounded on its own, in fp32:
 *   bits 8          torchvision's to_pil_image: pic.mul(255).byte() -- v * 255, truncated toward zero;
 *   bits 16         base.py:837: (t * 65535).clip(0, 65535).astype(uint16) -- v * 65535, truncated toward zero;
 *   encode_normal   base.py:818 first: (v + 1.0) * 0.5; channels must be 3.
 * Inside [0, 1] every sample is the reference's bit for bit.  Where the reference is undefined behaviour the result SATURATES: below 0
 * -> 0, above the maximum -> the maximum, +-inf likewise, NaN -> 0.  A map whose rows are dense, with width % 4 == 0, plane starts
 * 16-byte aligned and dst dword aligned is written in whole dwords, 4 pixels per lane; every other map one pixel per lane.  A launch
 * writes exactly height * width * channels samples per map and must not write what it reads.  No workspace, no atomics.  Caller errors,
 * before anything is launched: a NULL table, `src` or `dst` PBR_ERR_NULL_MAP; n_maps outside [1, PBR_MAX_IMAGE_PACKS], an extent < 1,
 * height * width > 2^40, a negative stride, a `src` that is not 4-byte aligned, a `dst` for 16 bit that is not 2-byte aligned, two `dst`
 * ranges of one call that overlap PBR_ERR_SHAPE; `bits` not 8 or 16 PBR_ERR_DTYPE; `channels` outside 1..4, or not 3 with
 * encode_normal, PBR_ERR_CHANNELS.  (ABI 9: an entry point added, nothing changed.)
 */
#define PBR_MAX_IMAGE_PACKS 8
typedef struct pbr_image_pack {
    const float *src;             /* planar float32; element strides below */
    int64_t stride_c, stride_h, stride_w;
    void *dst;                    /* dense (H, W, C) samples, uint8 or uint16 */
    int32_t channels;             /* 1..4; 3 when encode_normal */
    int32_t bits;                 /* 8 | 16 */
    int32_t encode_normal;        /* (v + 1) * 0.5 first */
    int32_t reserved;
} pbr_image_pack;
int pbr_pack_images(const pbr_image_pack *maps, int32_t n_maps, int32_t height, int32_t width, void *stream);

/*
 * Photograph rectification (no upstream counterpart; csrc/rectify.hip): n_images photographs, uint8 samples as PIL hands them out, are
 * warped onto the height x width texture grid by one 3x3 homography each, and come out as what the light-stack loss steps take:
 * targets [n_images][3][height][width] and coverage weights [n_images][height][width], float32, dense.  The definition, for output pixel
 * (y, x) of image l with M = homographies[l] (row-major), S = supersample and the sub-samples i, j < S:
 *   1. X = x + (i + 0.5) / S, Y = y + (j + 0.5) / S: output pixel centres sit at + 0.5, the grid spans [0, width] x [0, height];
 *   2. d = m20 X + m21 Y + m22, u = (m00 X + m01 Y + m02) / d - 0.5, v = (m10 X + m11 Y + m12) / d - 0.5: source pixel centres sit at
 *      + 0.5, so u, v are in index units;
 *   3. the sub-sample is OUTSIDE when d <= 0, u or v is not finite, u <= -1, u >= src_width, v <= -1 or v >= src_height;
 *   4. otherwise the bilinear taps at (floor u, floor v) and its three neighbours, weights from fx = u - floor u, fy = v - floor v.  A tap
 *      whose index lies outside the image contributes 0 (zeros padding: F.grid_sample(mode="bilinear", padding_mode="zeros",
 *      align_corners=False)); with clip_level = k in 1..255 a tap with any of its three samples >= k (an exact integer comparison)
 *      counts as outside the image too, in the value and in the coverage.
 *   value_c = sum of w_t * sample_tc / 255 over all taps of all sub-samples, / S^2; coverage = the sum of w_t over the same taps, / S^2;
 *   with to_linear every tap's sample / 255 goes through pbr_srgb_to_linear's function before it is weighted.
 *   weights = coverage, in [0, 1]; targets_c = clamp(value_c / coverage, 0, 1) where coverage > 0 and exactly 0 where coverage == 0, so a
 *   masked-out target is always finite.  No per-pixel threshold: value and coverage are continuous in the coordinates.
 * sample / 255 is the IEEE quotient of pbr_unpack_image: for a homography that is an integer translation, with S = 1, the targets are
 * pbr_unpack_image's floats bit for bit and the weights exactly 1 inside the image, exactly 0 outside.  The projective map is evaluated in
 * float64 (u = numerator * (1 / d): 1.5 ulp of a double), fx and fy are rounded to float32 after the floor, weights and sums are float32:
 * within (4 S^2 + 4) * 2^-24 <= 4.1e-6 of the definition in exact arithmetic, for source images of any size.
 * `src` is addressed as src[l*src_image_stride + y*src_stride_h + x*src_stride_w + c*src_stride_c] (strides in samples, none negative);
 * only channels c = 0..2 are read, so an RGBA array travels as it is (stride_w 4) and a dense RGB array has stride_w 3.  `homographies`
 * is HOST memory, [n_images][9], read at the call: the matrices travel in the kernel arguments (1152 bytes at most), ONE launch serves
 * all images.  A width % 4 == 0 with both outputs 16-byte aligned is written 4 pixels per lane, one 16-byte store per plane; everything
 * else one pixel per lane, with the same bits.  Every element of both outputs is written exactly once; no workspace, no atomics;
 * deterministic.  Caller errors, before anything is launched: a NULL pointer PBR_ERR_NULL_MAP; n_images outside
 * [1, PBR_MAX_RECTIFY_IMAGES], an extent < 1, height or width > 2^30, height * width > 2^40, supersample not 1, 2 or 4, clip_level outside
 * [0, 255] (0: off), a negative stride, a homography entry that is not finite PBR_ERR_SHAPE.  (ABI 9: an entry point added, nothing changed.)
 */
#define PBR_MAX_RECTIFY_IMAGES 16
int pbr_rectify_images(const void *src, int32_t n_images, int32_t src_height, int32_t src_width, int64_t src_image_stride,
                       int64_t src_stride_h, int64_t src_stride_w, int64_t src_stride_c, const double *homographies, float *targets,
                       float *weights, int32_t height, int32_t width, int32_t supersample, int32_t clip_level, int32_t to_linear,
                       void *stream);

/*
 * Photometric-stereo initialisation (no upstream counterpart; csrc/photometric.hip): a rectified light stack -- what pbr_rectify_images
 * writes -- becomes the maps a fit starts from, by a Lambertian least-squares solve per pixel with reweighting passes against attached
 * shadows.  Inputs: `targets` [n_shots][3][height][width] float32, dense; `weights` [n_shots][height][width], or ONE plane
 * [height][width] for all shots (weights_shared != 0), or NULL (every weight 1); `lights` and `intensities`, HOST memory, [n_shots][3]
 * floats each, read at the call (they travel in the kernel arguments: 16 x 6 values at most) -- point-light positions or directions
 * (light_type PBR_LIGHT_POINT | PBR_LIGHT_DIRECTIONAL) and the RGB intensity of every shot.  The definition, for output pixel (y, x) at
 * P = (xs[x], -ys[y], 0), xs and ys the point light's grid (linspace(-s/2, s/2, .) per axis in float32, s = light_size, 0 meaning 1.0,
 * exactly as pbr_cook_torrance forms it; cooktorrance.py:132-140):
 *   1. geometry per shot l.  Point light: d = light_l - P, w_l = d / (|d| + 1e-7), a_l = 1 / (|d|^2 + 1e-7).  Directional light:
 *      w_l = light_l / max(|light_l|, 1e-12), a_l = 1.
 *   2. observation per shot.  r_lc = lin(T_lc) / (I_lc a_l), lin = pbr_srgb_to_linear's function (input clamped to [0, 1]) with
 *      targets_srgb, the identity without; y_l = (r_l0 + r_l1 + r_l2) / 3.
 *   3. reweighted least squares.  m_l = 1; for pass k = 0 .. iterations - 1: u_l = weight_l m_l.  Shots with u_l == 0 are SKIPPED BY
 *      SELECTION, not multiplied: a NaN target under a zero weight does no harm (unlike the loss steps, where 0 * NaN is NaN).
 *      A = sum u_l w_l w_l^T, b = sum u_l y_l w_l; t = tr A; c = det A / (t/3)^3 if t > 0, else 0 (c is in [0, 1] by the AM-GM
 *      inequality).  c < min_condition: the pixel is INVALID, stop.  g = A^-1 b through the adjugate.  |g| zero or not finite, or
 *      g_z <= 0: INVALID, stop.  If k < iterations - 1: m_l = [w_l . g > shadow_cos |g|], the attached-shadow mask the current solution
 *      predicts.  (A pass whose mask equals the one before it repeats that pass: an implementation may stop there.)
 *   4. normal.  Valid: n = g / |g|, with u_l and c of the last pass.  Invalid: n = (0, 0, 1) exactly, and u_l = weight_l.
 *   5. albedo.  s_l = max(w_l . n, 0); albedo_c = clamp(pi sum u_l s_l r_lc / sum u_l s_l^2, 0, 1), exactly 0 where the denominator
 *      is 0 (shots with u_l == 0 skipped as in 3.); with albedo_srgb the result goes through pbr_linear_to_srgb's function.
 *   6. outputs, float32, dense: `normal` [3][height][width], the vector form a material's normal holds; `albedo` [3][height][width];
 *      `confidence` [height][width], c for a valid pixel and exactly 0 for an invalid one -- confidence > 0 is the validity mask, since
 *      min_condition > 0.
 * The solve is Lambertian and view-independent: no camera enters.  Arithmetic is float32 (hardware rcp, rsqrt, sqrt, log2, exp2 at
 * about 1 ulp each; 1 / I_lc is formed in double on the host); the error grows with 1 / c.  A width % 4 == 0 with all
 * five device pointers 16-byte aligned is read and written 4 pixels per lane, 16 bytes per access; everything else one pixel per lane,
 * with the same bits.  ONE launch; every element of the three outputs is written exactly once; no workspace, no atomics; deterministic.
 * Caller errors, before anything is launched: a NULL `targets`, `lights`, `intensities`, `normal`, `albedo` or `confidence`
 * PBR_ERR_NULL_MAP; n_shots outside [1, PBR_MAX_PHOTOMETRIC_SHOTS], an extent < 1, height or width > 2^30, height * width > 2^40,
 * iterations outside [1, 4], shadow_cos outside [0, 1), min_condition outside (0, 1), an unknown light_type, a light or intensity entry
 * (or, for a point light, a light_size) that is not finite, an intensity <= 0 PBR_ERR_SHAPE.  (ABI 9: an entry point added, nothing
 * changed.)
 */
#define PBR_MAX_PHOTOMETRIC_SHOTS 16
int pbr_photometric_stereo(const float *targets, const float *weights, int32_t weights_shared, int32_t n_shots, int32_t height,
                           int32_t width, const float *lights, const float *intensities, int32_t light_type, float light_size,
                           int32_t targets_srgb, int32_t iterations, float shadow_cos, float min_condition, int32_t albedo_srgb,
                           float *normal, float *albedo, float *confidence, void *stream);

/*
 * MaterialBase.resize, base.py:490-504 (torchvision resize of a float (C,H,W) map ==
 * F.interpolate(mode="bilinear", align_corners=False, antialias=...)).  fp32 planar
 * [planes][h_in][w_in] -> [planes][h_out][w_out]; `workspace` holds the width-pass
 * intermediate (or the row walk's tap tables), pbr_resize_workspace_bytes(planes, h_in, w_out) bytes of device memory, 16-byte aligned.
 */
size_t pbr_resize_workspace_bytes(int64_t planes, int32_t h_in, int32_t w_out);
int pbr_resize_bilinear(const void *src, void *dst, int64_t planes, int32_t h_in, int32_t w_in,
                        int32_t h_out, int32_t w_out, int antialias, void *workspace, void *stream);
/* Which kernel family pbr_resize_bilinear runs for these arguments under the current knobs (nothing is launched; -1 = the call would
 * fail): what a caller's test asserts when it compares two families bit for bit, what a profile's reader looks up.  ABI 8. */
enum {
    PBR_RESIZE_TWO_PASS = 0,            /* width pass, height pass through the workspace (more than 36 taps per axis; csrc/resize.hip) */
    PBR_RESIZE_STRIP = 1,               /* one kernel, tile by tile through an LDS strip (csrc/resize_strip.hpp: resize_strip_kernel) */
    PBR_RESIZE_TWO_TAP = 2,             /* up-scales on both axes, registers only (csrc/resize.hip: resize_up2_kernel) */
    PBR_RESIZE_BAND_WALK = 3,           /* antialiased whole factors 2 ... 8 | 16, registers only (csrc/resize_down.hpp) */
    PBR_RESIZE_ROW_WALK = 4             /* other antialiased down-scales from 7 x up, i.e. 17 ... 36 taps per axis (every one from 1.01 x to 17 x with the knob PBR_TUNE_RESIZE_UP2 at 2): every input row read once (csrc/resize_stream.hpp) */
};
int pbr_resize_form(const void *src, const void *dst, int64_t planes, int32_t h_in, int32_t w_in, int32_t h_out,
                    int32_t w_out, int antialias, const void *workspace);

/*
 * Gradient of pbr_resize_bilinear w.r.t. its input (autograd through base.py:490-504 -> F.interpolate): the transposed tap
 * matrices, g_in = Wy^T g_out Wx, gathered by input index in a fixed order (deterministic, no atomics; csrc/resize_backward.hip).  grad_out
 * [planes][h_out][w_out] -> grad_in [planes][h_in][w_in], fp32; `workspace`: pbr_resize_backward_workspace_bytes(...) bytes.
 */
size_t pbr_resize_backward_workspace_bytes(int64_t planes, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out);
int pbr_resize_bilinear_backward(const void *grad_out, void *grad_in, int64_t planes, int32_t h_in, int32_t w_in, int32_t h_out,
                                 int32_t w_out, int antialias, void *workspace, void *stream);

/*
 * Material blending in front of the BRDF (examples/example_blend.py:14-16), fp32 planar maps.
 * pbr_blend_maps: blend_with_mask blending/functional.py:64-116 for ONE map, out = mask * map1 +
 * (1 - mask) * map2 over [channels][pixels] with a [pixels] mask; is_normal selects _blend_normals
 * (:119-145: normalise both, blend, re-normalise; 3 channels).
 * pbr_blend_sigmoid_mask: the mask of blend_on_height / blend_on_properties (:148-239),
 * sigmoid((prop1 + shift - prop2) / (blend_width + 1e-6)).
 * pbr_blend_gradient_mask: the mask of blend_with_gradient (:242-286), linspace(0,1) along x
 * (vertical = 0) or y (vertical = 1), shape [height][width].
 */
int pbr_blend_maps(const void *map1, const void *map2, const void *mask, void *out, int32_t channels,
                   int64_t pixels, int is_normal, void *stream);
/* Gradient of pbr_blend_maps (autograd through functional.py:103-110 / :119-145): g_map1, g_map2 [channels][pixels] and
 * g_mask [pixels], any of them NULL = not wanted; accumulate_mask: g_mask += (a material's maps share one mask). */
int pbr_blend_maps_backward(const void *map1, const void *map2, const void *mask, const void *grad_out, void *g_map1,
                            void *g_map2, void *g_mask, int32_t channels, int64_t pixels, int is_normal,
                            int accumulate_mask, void *stream);
int pbr_blend_sigmoid_mask(const void *prop1, const void *prop2, void *mask, int64_t n, float shift,
                           float blend_width, void *stream);
/* Gradient of pbr_blend_sigmoid_mask w.r.t. both property maps (autograd through torch.sigmoid, functional.py:184-193), from the
 * mask the forward call produced: g_prop1 = grad_out * mask (1 - mask) / (blend_width + 1e-6), g_prop2 = -g_prop1; NULL = not wanted. */
int pbr_blend_sigmoid_mask_backward(const void *mask, const void *grad_out, void *g_prop1, void *g_prop2, int64_t n, float blend_width,
                                    void *stream);
int pbr_blend_gradient_mask(void *mask, int32_t height, int32_t width, int vertical, void *stream);

/* ---- the optimiser step of a fit (csrc/adam.hip; pypbr_amd.optim.MaterialAdam) ------ */

/*
 * Projected Adam over a table of at most PBR_MAX_ADAM_TENSORS tensors, ONE launch.  Per element, with the coefficients of the entry's
 * group (a = lr / (1 - beta1^t), c = 1 / sqrt(1 - beta2^t), formed in float64 by the caller or by pbr_adam_advance):
 *     m <- m + (g - m) (1 - beta1)        v <- beta2 v + (1 - beta2) g g        delta = a m / (sqrt(v) c + eps)        p <- p - delta
 * -- torch.optim.Adam (weight_decay 0, no amsgrad, no maximize) in exact arithmetic -- and then the entry's projection of p:
 *   PBR_ADAM_NONE   nothing
 *   PBR_ADAM_BOX    min(max(p, lo), hi); -INFINITY / +INFINITY leave a side open
 *   PBR_ADAM_UNIT   (channels == 3) z <- max(z, min_z) (-INFINITY: no floor), then p / max(|p|, 1e-12) over the pixel's three planes
 * An element whose delta is exactly 0 (for UNIT: all three of the pixel) keeps the bits of its parameter: it is neither clamped nor
 * renormalised (a pixel no gradient ever reached).  Non-finite gradients propagate.  m, v (and `master`) are dense fp32 in the
 * parameter's logical order [batch][channels][pixels]; the parameter and its gradient, of the entry's `dtype`, have dense planes of
 * `pixels` elements at the given plane / batch strides (in elements).  PBR_F16 parameters carry an fp32 `master` copy: the update and the
 * projection run on the master, and the parameter receives the master rounded to nearest even in the same pass (an element that keeps
 * its bits keeps the master's too); PBR_F32 parameters pass master = NULL.  Every element of p, m, v, master is read once and written
 * once, g is read once.  Accesses are 16 bytes wide (8 for fp16) for an entry whose pointers, strides and `pixels` are whole quads,
 * element by element otherwise.
 * The coefficients: `coeffs_host` (n_groups rows, copied into the kernel's arguments) or `coeffs_device` (n_groups rows of device memory
 * the kernel reads when it RUNS: a captured graph replays with whatever pbr_adam_advance wrote there) -- exactly one of the two.
 * Caller errors, before anything is launched: a NULL table, both or neither coefficient table, a NULL p / g / m / v, a PBR_F16 entry
 * without master PBR_ERR_NULL_MAP; n_tensors or n_groups outside [1, PBR_MAX_ADAM_TENSORS], batch / channels / pixels < 1, a negative
 * stride, planes or images of p on top of each other, lo > hi, a group index outside the table, a pointer off its element's alignment,
 * anything written that overlaps anything else the launch reads or writes (p and g of one entry included) PBR_ERR_SHAPE; UNIT with
 * channels != 3 PBR_ERR_CHANNELS; an unknown projection, a master behind a PBR_F32 entry PBR_ERR_UNSUPPORTED; a dtype PBR_ERR_DTYPE.
 * No workspace.  (ABI 9: entry points added, nothing changed.)
 */
enum { PBR_ADAM_NONE = 0, PBR_ADAM_BOX = 1, PBR_ADAM_UNIT = 2 };
#define PBR_MAX_ADAM_TENSORS 16
#define PBR_ADAM_BLOCK 256            /* lanes of a workgroup; a lane takes one quad (or one element) of a plane per trip of its loop */
#define PBR_ADAM_MAX_BLOCKS 1024      /* workgroups per tensor at the most: planes of more than 256 x 1024 quads make a lane loop */
typedef struct pbr_adam_tensor {
    void *param;
    const void *grad;
    float *exp_avg;               /* m */
    float *exp_avg_sq;            /* v */
    float *master;                /* PBR_F16: the fp32 copy the update runs on; PBR_F32: NULL */
    int64_t pixels;               /* elements of one plane */
    int64_t param_batch_stride, param_plane_stride;
    int64_t grad_batch_stride, grad_plane_stride;
    int32_t batch, channels;
    int32_t dtype;                /* PBR_F32 | PBR_F16: param and grad */
    int32_t project;              /* PBR_ADAM_* */
    float lo, hi;                 /* BOX */
    float min_z;                  /* UNIT */
    int32_t group;                /* row of the coefficient table */
} pbr_adam_tensor;
typedef struct pbr_adam_coeffs {
    float a, c, one_minus_beta1, beta2, one_minus_beta2, eps;
} pbr_adam_coeffs;
int pbr_adam_step(const pbr_adam_tensor *tensors, int32_t n_tensors, const pbr_adam_coeffs *coeffs_host, const void *coeffs_device,
                  int32_t n_groups, void *stream);
/* What pbr_adam_step checks about its table before it launches, alone: PBR_OK, or the caller error it would return.  Launches nothing.
 * The overlap test is exact for strided entries (plane by plane where the planes are not back to back): the maps of a batch packed
 * material by material interleave -- material 0's normal lies between material 0's and material 1's albedo -- and are accepted. */
int pbr_adam_check(const pbr_adam_tensor *tensors, int32_t n_tensors, int32_t n_groups);
/* sizeof(pbr_adam_tensor) as compiled: bindings check their struct layout against it. */
size_t pbr_adam_tensor_size(void);
/*
 * The step counters of a capturable optimiser, ONE lane: for every row i < n_groups, *step <- *step + 1 (a DEVICE float, torch's
 * capturable `step`; every counter appears in one row only), t = the new value, and row i of `coeffs_device` (pbr_adam_coeffs) receives
 * a = lr / (1 - beta1^t), c = 1 / sqrt(1 - beta2^t), formed in float64 on the device and rounded once, with 1 - beta1, beta2, 1 - beta2
 * and eps.  lr is `lr`, or -- `lr_device` not NULL -- the DEVICE float it points to, read when the kernel runs.  The only place where t
 * enters: a captured graph of pbr_adam_advance + pbr_adam_step(coeffs_device) replays correctly.  A NULL table, counter or coefficient
 * table PBR_ERR_NULL_MAP; n_groups outside [1, PBR_MAX_ADAM_TENSORS] PBR_ERR_SHAPE.
 */
typedef struct pbr_adam_group {
    void *step;
    const void *lr_device;
    double lr, beta1, beta2, eps;
} pbr_adam_group;
int pbr_adam_advance(const pbr_adam_group *groups, int32_t n_groups, void *coeffs_device, void *stream);

/* ---- the smoothness prior of a fit (csrc/smoothness.hip; pypbr_amd.priors) ---------- */

/*
 * Vectorial total variation / Tikhonov over a table of at most PBR_MAX_SMOOTH_TENSORS maps: value and gradients of all of them in ONE
 * launch (and one small finish launch).  No upstream counterpart; tools/smoothness_oracle.py is the definition in float64 numpy.
 * For one entry, planes p[b][c][y][x], B x C x H x W, 1 <= C <= 4:
 *   forward differences   dx_c(y,x) = p_c(y,x+1) - p_c(y,x),  dy_c(y,x) = p_c(y+1,x) - p_c(y,x).  wrap = 0: a difference that would reach
 *                         outside the map is exactly 0; wrap = 1: indices modulo W and H (tileable textures; consistent with roll / tile)
 *   channel coupling      s(y,x) = sum_c (dx_c^2 + dy_c^2)
 *   penalty               PBR_SMOOTH_L2: phi = s.  PBR_SMOOTH_CHARBONNIER: phi = sqrt(s + eps^2) - eps, eps > 0, evaluated as
 *                         s / (sqrt(s + eps^2) + eps) (the difference cancels in float32)
 *   value                 R = k sum_{b,y,x} w(b,y,x) phi(s(b,y,x)); k is the caller's (lambda / (B H W) for a mean, lambda for a sum),
 *                         w an optional float32 plane per image (weights_batch_stride 0: one shared by the batch), 1 where absent.  A
 *                         weight multiplies, it does not skip: a NaN parameter under a weight of 0 still reaches its neighbours.
 *   gradient              q = k w 2 phi'(s)  (2 for L2, 1 / sqrt(s + eps^2) for Charbonnier),
 *                         g_c(y,x) = -q(y,x) (dx_c(y,x) + dy_c(y,x)) + q(y,x-1) dx_c(y,x-1) + q(y-1,x) dy_c(y-1,x), terms outside the
 *                         map 0, or wrapped
 * *loss receives the sum of the entries' R, terms[i] (NULL: not wanted) entry i's R.  `grad` (NULL: value only) is WRITTEN, not
 * accumulated into, in the map's dtype (PBR_F32 | PBR_F16; arithmetic in fp32).  Rows are dense; batch and plane strides in elements.
 * One pass: a wave walks down a strip of 63 units of a band of at most PBR_SMOOTH_BAND_ROWS rows (halved, down to
 * PBR_SMOOTH_MIN_BAND_ROWS, while the launch has fewer than PBR_SMOOTH_MIN_BLOCKS workgroups) -- a unit is four pixels when the width,
 * the strides and the pointers of the entry are whole quads, else one pixel -- with one halo unit on its left and one halo row above,
 * so every (q dx_c, q dy_c) is formed once per strip and every gradient value is written once.  The value is reduced without atomics:
 * one fp32 partial per workgroup in `workspace`, summed in fp64 in a fixed order by the finish launch: two runs give the same bits.
 * Caller errors, before anything is launched: a NULL table, param, loss or workspace PBR_ERR_NULL_MAP; n outside
 * [1, PBR_MAX_SMOOTH_TENSORS], batch / height / width < 1, height or width > 2^30, height * width > 2^40, more than 2^31 - 1 workgroups,
 * a negative stride, eps <= 0 (or not finite) with Charbonnier, a k that is not finite, a pointer off its element's alignment, a
 * workspace smaller than pbr_smoothness_workspace_bytes, a `grad` that overlaps any param, weights or other grad of the launch (tested
 * plane by plane, as pbr_adam_check does) PBR_ERR_SHAPE; channels outside 1..4 PBR_ERR_CHANNELS; an unknown kind PBR_ERR_UNSUPPORTED; a
 * dtype PBR_ERR_DTYPE.  (ABI 9: entry points added, nothing changed.)
 */
enum { PBR_SMOOTH_L2 = 0, PBR_SMOOTH_CHARBONNIER = 1 };
#define PBR_MAX_SMOOTH_TENSORS 8
#define PBR_SMOOTH_BLOCK 256          /* lanes of a workgroup: 4 waves, 4 adjacent strips of 63 units (+ 1 halo unit) each */
#define PBR_SMOOTH_BAND_ROWS 32       /* rows of a band at the most (+ 1 halo row above, 1 row read below) */
#define PBR_SMOOTH_MIN_BAND_ROWS 4    /* ... and at the least: the bands of a launch are halved while it has fewer than */
#define PBR_SMOOTH_MIN_BLOCKS 512     /* ... this many workgroups */
typedef struct pbr_smooth_tensor {
    const void *param;
    void *grad;                   /* NULL: value only */
    const float *weights;         /* NULL: 1 everywhere */
    int64_t param_batch_stride, param_plane_stride;
    int64_t grad_batch_stride, grad_plane_stride;
    int64_t weights_batch_stride; /* 0: one plane shared by the batch */
    double k;                     /* formed in float64 by the caller; the gradient uses it rounded to fp32 */
    float eps;                    /* CHARBONNIER */
    int32_t dtype;                /* PBR_F32 | PBR_F16: param and grad */
    int32_t batch, channels, height, width;
    int32_t kind;                 /* PBR_SMOOTH_* */
    int32_t wrap;
} pbr_smooth_tensor;
int pbr_smoothness_step(const pbr_smooth_tensor *tensors, int32_t n_tensors, void *loss, void *terms, void *workspace, size_t workspace_bytes,
                        void *stream);
/* Bytes of workspace pbr_smoothness_step needs for this table (one fp32 per workgroup); 0 for a table pbr_smoothness_check refuses. */
size_t pbr_smoothness_workspace_bytes(const pbr_smooth_tensor *tensors, int32_t n_tensors);
/* What pbr_smoothness_step checks about its table before it launches, alone: PBR_OK, or the caller error.  Launches nothing. */
int pbr_smoothness_check(const pbr_smooth_tensor *tensors, int32_t n_tensors);
/* sizeof(pbr_smooth_tensor) as compiled: bindings check their struct layout against it. */
size_t pbr_smooth_tensor_size(void);

/* ---- introspection; the process-global tuning hook (tests, benches, profiling) ------ */
int pbr_abi_version(void);
/* First 16 hex digits of the SHA-256 over the sources this library was built from (every .hip and .hpp file of csrc, this header, the Makefile,
 * in sorted order): evidence files carry it, and collectors refuse a library that is not the one the sources next to it would build. */
const char *pbr_build_id(void);
/* sizeof(pbr_render_desc) as compiled: bindings check their struct layout against it. */
size_t pbr_render_desc_size(void);
const char *pbr_error_string(int code);
/* Name of the kernel the descriptor dispatches to (no launch); NULL on a bad descriptor. */
const char *pbr_kernel_name(const pbr_render_desc *desc);
/* Algorithmic HBM bytes per pixel of that dispatch: reads + writes. */
int pbr_bytes_per_pixel(const pbr_render_desc *desc);
/* The process-global hook behind the knobs above (pbr_tuning): sets the value every later call of the PROCESS uses for `knob`
 * unless its descriptor overrides it; returns the previous value, -1 for an unknown knob.  For tests, benches and profiling runs
 * (the Python binding feeds PBR_TUNE_* environment variables through it at load).  Atomic, so it may be called while other threads
 * launch; it is still shared state -- a knob left set changes which kernel a later, unrelated caller gets (never its results) --
 * which is why product code uses pbr_render_desc.tuning.  pbr_set_tuning(knob, PBR_TUNE_UNSET) restores the rule. */
int pbr_set_tuning(int knob, int value);

#ifdef __cplusplus
}
#endif
#endif /* PBR_HIP_H */
