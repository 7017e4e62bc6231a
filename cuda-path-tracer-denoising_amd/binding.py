"""ctypes binding of libsvgf_hip.so (include/svgf.h) and a host-side mirror of the reference interface.

The reference's interface for this path is three free functions over global state
(reference src/denoise.h:6-8): denoiseInit(scene) / denoise(out, in, gbuffer) / denoiseFree(), with the tunables
in `ui_*` globals (src/main.h:39-69).  `Denoiser` keeps those names and meanings:
    d = Denoiser(width, height, device=0)     # denoiseInit
    d.ui.temporal_enable = 1 ...              # the ui_* block
    d.denoise(out, inp, gbuffer, camera)      # denoise (device pointers / torch tensors)
    d.free()                                  # denoiseFree
There is NO CPU fallback: if the HIP library is missing or no GPU is present, construction raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsvgf_hip.so")
LIB_EXP_PATH = os.path.join(_HERE, "libsvgf_hip_exp.so")     # -DSVGF_BUILD_EXPERIMENTS: parked variants + tuning table (tests / tools only)

SVGF_OK = 0
STATE_HISTORY_LENGTH, STATE_MOMENTS, STATE_COLOR_HISTORY, STATE_VARIANCE_TEMPORAL, STATE_COLOR_ACC = range(5)
# what the NEXT frame reads of the previous G-buffer, and svgf_set_output_taa's history (svgf_transfer_history moves all of them)
STATE_PREV_NORMAL, STATE_PREV_POSITION, STATE_PREV_GEOM_ID, STATE_OUTPUT_HISTORY = 5, 6, 7, 8
KERNEL_TEMPORAL, KERNEL_PREPARE, KERNEL_ATROUS, KERNEL_DEBUGVIEW, KERNEL_COPYOUT, KERNEL_FUSED, KERNEL_OUTPUT_TAA = 1, 2, 3, 4, 5, 6, 7
MAX_LEVELS = 10
# svgf_exp_level_kernels (experiments build): the kernel an a-trous level ran
LEVEL_KERNEL_NAMES = ("fused", "lane", "lane2y", "strip", "lattice", "gather")

# every symbol include/svgf_trace.h declares (libsvgf_trace.so, the companion library of row f17)
TRACE_EXPORTS = ["svgf_trace_draw", "svgf_trace_version"]
# libsvgf_split.so (include/svgf_split.h, row f18)
SPLIT_EXPORTS = ["svgf_trace_draw_split", "svgf_trace_compose"]
TRACE_MAX_BOUNCE_SAMPLES = 8
# libsvgf_path.so (include/svgf_path.h, row f19)
PATH_EXPORTS = ["svgf_path_draw", "svgf_path_draw_split", "svgf_path_version"]
PATH_MAX_PATHS = 8
PATH_MAX_DEPTH = 8
# libsvgf_gloss.so (include/svgf_gloss.h, row f20)
GLOSS_EXPORTS = ["svgf_gloss_table_create", "svgf_gloss_table_destroy", "svgf_gloss_table_size", "svgf_gloss_draw", "svgf_gloss_draw_split",
                 "svgf_gloss_version"]
# libsvgf_virtual.so (include/svgf_virtual.h, row f21)
VIRTUAL_EXPORTS = ["svgf_virtual_draw", "svgf_virtual_draw_split", "svgf_virtual_version"]
# libsvgf_rough.so (include/svgf_rough.h, row f22)
ROUGH_EXPORTS = ["svgf_rough_table_create", "svgf_rough_table_destroy", "svgf_rough_table_size", "svgf_rough_draw", "svgf_rough_draw_split",
                 "svgf_rough_version"]
# libsvgf_highlight.so (include/svgf_highlight.h, row f23)
HIGHLIGHT_EXPORTS = ["svgf_highlight_draw", "svgf_highlight_draw_split", "svgf_highlight_version"]
# libsvgf_lbvh.so (include/svgf_lbvh.h, row f24): the device BVH builder - built by the companions' recipe (build.BUILDERS) and linked
# like them, but no companion draw: not a row of COMPANIONS (its symbols: LBVH_EXPORTS, below the structures)
LIB_LBVH_PATH = os.path.join(_HERE, "libsvgf_lbvh.so")
LBVH_READ_NODES, LBVH_READ_ORDER, LBVH_READ_KEYS = 0, 1, 2
LBVH_TILE = 512
# The companion libraries in the order they were added (build.COMPANIONS is the builder's side of this table): the short name
# (libsvgf_<name>.so, include/svgf_<name>.h) and every symbol the header declares.
Companion = collections.namedtuple("Companion", "name exports")
COMPANIONS = (Companion("trace", TRACE_EXPORTS), Companion("split", SPLIT_EXPORTS), Companion("path", PATH_EXPORTS), Companion("gloss", GLOSS_EXPORTS),
              Companion("virtual", VIRTUAL_EXPORTS), Companion("rough", ROUGH_EXPORTS), Companion("highlight", HIGHLIGHT_EXPORTS))


def companion_path(name: str) -> str:
    return os.path.join(_HERE, f"libsvgf_{name}.so")


def companion_exports(name: str) -> list[str]:
    return next(c.exports for c in COMPANIONS if c.name == name)


LIB_TRACE_PATH, LIB_SPLIT_PATH, LIB_PATH_PATH, LIB_GLOSS_PATH, LIB_VIRTUAL_PATH, LIB_ROUGH_PATH, LIB_HIGHLIGHT_PATH = (companion_path(c.name) for c in COMPANIONS)
SCENE_MAX_DEPTH = 48
SCENE_MAX_POSED = 1024
SCENE_REFIT_CAP = 1024
SCENE_MAX_SHADOW_SAMPLES = 64
# svgf_scene_read kinds
SCENE_READ_TRIS, SCENE_READ_TRI_BOXES, SCENE_READ_NODES, SCENE_READ_GEOMS, SCENE_READ_ORDER, SCENE_READ_HELD_POSE = 0, 1, 2, 3, 4, 5
# SvgfScenePose / SvgfRefitTreelet (row f15)
SCENE_POSE_DTYPE = np.dtype([("xf", np.float32, (12,)), ("inv", np.float32, (12,))])
REFIT_TREELET_DTYPE = np.dtype([("root", np.int32), ("begin", np.int32), ("count", np.int32), ("levels", np.int32)])
CREATE_PIPELINED = 1
EXPOSURE_STATE_WORDS = 520
# SvgfTonemapParams.op / .transfer
TONEMAP_NONE, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2
TRANSFER_LINEAR, TRANSFER_GAMMA2, TRANSFER_SRGB = 0, 1, 2
# motion plane formats (svgf_denoise_motion): absolute previous coordinate, delta in float32, delta in float16
MOTION_PREV_COORD_F32, MOTION_DELTA_F32, MOTION_DELTA_F16 = 1, 2, 3


class SvgfCamera(C.Structure):
    _fields_ = [("right", C.c_float * 3), ("up", C.c_float * 3), ("view", C.c_float * 3), ("position", C.c_float * 3)]

    @classmethod
    def from_dict(cls, d):
        c = cls()
        for k in ("right", "up", "view", "position"):
            for i in range(3):
                getattr(c, k)[i] = float(d[k][i])
        return c


class SvgfParams(C.Structure):
    _fields_ = [("temporal_enable", C.c_int), ("spatial_enable", C.c_int), ("color_alpha", C.c_float),
                ("moment_alpha", C.c_float), ("blur_variance", C.c_int), ("sigma_l", C.c_float),
                ("sigma_x", C.c_float), ("sigma_n", C.c_float), ("atrous_nlevel", C.c_int),
                ("history_level", C.c_int), ("sepcolor", C.c_int), ("addcolor", C.c_int),
                ("right_view_option", C.c_int), ("kernel_variant", C.c_int), ("inputs_ready", C.c_int),
                ("reproj_scale", C.c_float * 2), ("paper_steps", C.c_int), ("reproj_position_tol", C.c_float),
                ("spatial_variance_frames", C.c_int)]

    def set(self, **kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)
        return self


class SvgfPlanarGBuffer(C.Structure):
    """Device pointers of the context's current-frame planes (svgf_planar_gbuffer): packed float3 normal / position / albedo,
    int geomId."""
    _fields_ = [("normal", C.c_void_p), ("position", C.c_void_p), ("geom_id", C.c_void_p), ("albedo", C.c_void_p)]


class SvgfGuide(C.Structure):
    """One resolution's G-buffer for svgf_upsample: device pointers of AoS texels (`gbuffer`, wins when set) or of the planes of
    svgf_planar_gbuffer's layout; `albedo` (albedo * ialbedo) is only read on the hi side with modulate."""
    _fields_ = [("gbuffer", C.c_void_p), ("normal", C.c_void_p), ("position", C.c_void_p), ("geom_id", C.c_void_p), ("albedo", C.c_void_p)]


class SvgfUpsampleParams(C.Structure):
    _fields_ = [("sigma_n", C.c_float), ("sigma_x", C.c_float), ("modulate", C.c_int)]


class SvgfExposureParams(C.Structure):
    """svgf_exposure_meter: the metered average is mapped to `key`; trims in 1/1024 of the counted pixels; `adapt` is the share of
    the way to the target taken per metering."""
    _fields_ = [("key", C.c_float), ("trim_low_1024", C.c_int), ("trim_high_1024", C.c_int), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("adapt", C.c_float)]


class SvgfTonemapParams(C.Structure):
    _fields_ = [("op", C.c_int), ("transfer", C.c_int), ("exposure_bias", C.c_float), ("white", C.c_float)]


class SvgfQualityParams(C.Structure):
    """svgf_quality_meter: `peak` is the signal's white, `scale` multiplies both images first, `clamp` = 1 clamps to [0, peak]."""
    _fields_ = [("peak", C.c_float), ("scale", C.c_float), ("clamp", C.c_int)]


class SvgfQualityResult(C.Structure):
    """svgf_quality_read: the eight device words, then the three quotients formed on the host."""
    _fields_ = [("n_pixels", C.c_ulonglong), ("n_windows", C.c_ulonglong), ("sum_se", C.c_double), ("sum_ssim", C.c_double),
                ("max_abs", C.c_double), ("min_ssim", C.c_double), ("peak", C.c_double), ("scale", C.c_double),
                ("mse", C.c_double), ("psnr_db", C.c_double), ("mean_ssim", C.c_double)]


class SvgfSceneBuildParams(C.Structure):
    """svgf_scene_create / svgf_bvh_build_host: max_leaf_tris 1..8 (0 = 4); split 0 = binned SAH, 1 = equal counts."""
    _fields_ = [("max_leaf_tris", C.c_int), ("split", C.c_int)]


class SvgfSceneInfo(C.Structure):
    _fields_ = [("n_geoms", C.c_int), ("n_tris", C.c_int), ("n_tex", C.c_int), ("n_nodes", C.c_int), ("n_leaves", C.c_int),
                ("depth", C.c_int), ("max_leaf_tris", C.c_int), ("device_bytes", C.c_ulonglong)]


class SvgfSceneLight(C.Structure):
    """svgf_scene_draw_shadowed: a parallelogram light centre +- edge_u +- edge_v (both edges zero: a point light) and the number of
    shadow rays per pixel and frame, 1..SCENE_MAX_SHADOW_SAMPLES."""
    _fields_ = [("centre", C.c_float * 3), ("edge_u", C.c_float * 3), ("edge_v", C.c_float * 3), ("samples", C.c_int)]

    @classmethod
    def make(cls, centre, edge_u=(0, 0, 0), edge_v=(0, 0, 0), samples: int = 1):
        l = cls()
        for i in range(3):
            l.centre[i], l.edge_u[i], l.edge_v[i] = float(centre[i]), float(edge_u[i]), float(edge_v[i])
        l.samples = int(samples)
        return l


class SvgfSceneView(C.Structure):
    """svgf_scene_view: the device pointers the draws read (the posed arrays on a posed scene), valid until svgf_scene_destroy or
    svgf_scene_enable_pose."""
    _fields_ = [("device", C.c_int), ("n_geoms", C.c_int), ("n_tris", C.c_int), ("n_tex", C.c_int), ("n_nodes", C.c_int), ("depth", C.c_int),
                ("geoms", C.c_void_p), ("geom_ids", C.c_void_p), ("tris", C.c_void_p), ("tri_ids", C.c_void_p), ("tri_albedo", C.c_void_p),
                ("tri_tex", C.c_void_p), ("tex_desc", C.c_void_p), ("tex", C.c_void_p), ("nodes", C.c_void_p), ("order", C.c_void_p),
                ("tri_boxes", C.c_void_p)]


class SvgfTraceParams(C.Structure):
    """svgf_trace_draw: directions gathered per pixel (0..TRACE_MAX_BOUNCE_SAMPLES), the constant term, and whether the bounce's hit
    casts a shadow ray of its own."""
    _fields_ = [("bounce_samples", C.c_int), ("ambient", C.c_float), ("shadow_secondary", C.c_int)]


class SvgfPathParams(C.Structure):
    """svgf_path_draw / svgf_path_draw_split: paths per pixel (0..PATH_MAX_PATHS), bounces per path (1..PATH_MAX_DEPTH), the bounce
    from which Russian roulette acts (0: never), the constant term, and whether the vertices behind the first cast a shadow ray."""
    _fields_ = [("paths", C.c_int), ("max_depth", C.c_int), ("rr_depth", C.c_int), ("ambient", C.c_float), ("shadow_secondary", C.c_int)]


class SvgfSurface(C.Structure):
    """One record of a svgf_gloss_table (include/svgf_gloss.h, row f20), 24 bytes: the mirror lobe's probability, > 0 for glass on a
    cube / sphere, the index of refraction, and the weight of a mirror / Fresnel reflection."""
    _fields_ = [("reflect", C.c_float), ("refract", C.c_float), ("ior", C.c_float), ("spec", C.c_float * 3)]


class SvgfVirtualParams(C.Structure):
    """svgf_virtual_draw / svgf_virtual_draw_split (include/svgf_virtual.h, row f21): the most rays the guide chain may trace
    (1..PATH_MAX_DEPTH) and the offset added to the geomId of a virtual hit (0..1 << 24)."""
    _fields_ = [("max_chain", C.c_int), ("id_offset", C.c_int)]


class SvgfRoughParams(C.Structure):
    """svgf_rough_draw / svgf_rough_draw_split (include/svgf_rough.h, row f22): the guide follows a full mirror whose roughness is at
    most guide_alpha (>= 0)."""
    _fields_ = [("guide_alpha", C.c_float)]


class SvgfHighlightParams(C.Structure):
    """svgf_highlight_draw / svgf_highlight_draw_split (include/svgf_highlight.h, row f23): enable 0 (the rough draws) or 1 (the
    light's GGX term at rough vertices), and the clamp of the scalar highlight factor (0: none)."""
    _fields_ = [("enable", C.c_int), ("clamp", C.c_float)]


# SvgfBvhNode, 32 bytes: count > 0 a leaf over order[first : first + count], count == 0 an inner node with children first, first + 1
BVH_NODE_DTYPE = np.dtype([("lo", np.float32, 3), ("first", np.int32), ("hi", np.float32, 3), ("count", np.int32)])


class SvgfSynthParams(C.Structure):
    _fields_ = [("frame", C.c_int), ("seed", C.c_int), ("noise", C.c_float), ("fireflies", C.c_float),
                ("pixel_length", C.c_float * 2)]


def reference_defaults() -> SvgfParams:
    """ui_* defaults of reference src/main.cpp:49-62 (pure Python copy; the library's svgf_params_default is
    checked against this in tests)."""
    p = SvgfParams()
    p.set(temporal_enable=0, spatial_enable=0, color_alpha=0.2, moment_alpha=0.2, blur_variance=1, sigma_l=0.45,
          sigma_x=0.35, sigma_n=0.2, atrous_nlevel=5, history_level=1, sepcolor=0, addcolor=0, right_view_option=0)
    return p


class SvgfError(RuntimeError):
    pass


class SvgfLbvhParams(C.Structure):
    _fields_ = [("leaf_tris", C.c_int)]


class SvgfLbvhInfo(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("n_tris", "n_leaves", "n_nodes", "leaf_tris", "idx_bits", "axis_bits", "key_bits", "depth_bound",
                                       "launches")] + [("device_bytes", C.c_ulonglong)]


def _check(rc, symbol, message=None):
    """The return-code check of every wrapper outside Denoiser (whose _check adds the context's last error)."""
    if rc != SVGF_OK:
        raise SvgfError(message or f"{symbol} failed ({rc})")


def _call(lib, symbol, *args):
    _check(getattr(lib, symbol)(*args), symbol)


def _ptr(x):
    """device pointer of a torch tensor / int / None"""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise SvgfError("tensor must be contiguous")
        return x.data_ptr()
    raise TypeError(type(x))


def _stream(stream):
    """raw handle of a torch stream / int / None"""
    return None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)


def _camera(camera):
    return camera if isinstance(camera, SvgfCamera) else SvgfCamera.from_dict(camera)


def _view(camera, width, height, frame, seed, noise, fireflies, pixel_length, camera_fovy):
    """(SvgfCamera, SvgfSynthParams) of a producer call.  pixel_length defaults to synth._pixel_length(width, height, field of view), so
    that host and device producers agree; the field of view is a camera dict's "fovy_deg" where `camera_fovy` (the scene entry points),
    and 45 degrees otherwise: for an SvgfCamera, a dict without the key, and the synth_render pair whatever the camera says."""
    if pixel_length is None:
        from . import synth as _synth
        fovy = camera.get("fovy_deg", 45.0) if camera_fovy and isinstance(camera, dict) else 45.0
        pixel_length = _synth._pixel_length(width, height, fovy)
    return _camera(camera), SvgfSynthParams(int(frame), int(seed), float(noise), float(fireflies), (float(pixel_length[0]), float(pixel_length[1])))


def _draw_target(out_gbuffer):
    """(planar?, AoS texels or None, planes by reference or None) of a G-buffer output: device memory or a SvgfPlanarGBuffer."""
    planar = isinstance(out_gbuffer, SvgfPlanarGBuffer)
    return planar, None if planar else _ptr(out_gbuffer), C.byref(out_gbuffer) if planar else None


def _v3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


# Every symbol include/svgf.h declares, in the order they were added: (restype, argtypes or None where none is declared).  load_library
# declares them from here and EXPORTS is this table's keys (tests/test_abi.py holds them against the header, tests/test_binding_surface.py
# the prototypes against tests/golden/binding_abi.json), so a symbol cannot be exported without its prototype.
def _prototypes():
    vp, ip, fl, P = C.c_void_p, C.c_int, C.c_float, C.POINTER
    fp, cam, synth, planes = P(fl), P(SvgfCamera), P(SvgfSynthParams), P(SvgfPlanarGBuffer)
    mesh = [vp, ip, vp, vp, vp, vp, ip, vp, vp, vp, ip]      # geoms, n, geom_ids, tris, tri_ids, tri_albedo, n, tri_tex, tex_desc, texels, n
    product = {
        "svgf_version": (ip, None),
        "svgf_params_default": (ip, [P(SvgfParams)]),
        "svgf_create": (ip, [ip, ip, ip, P(vp)]),
        "svgf_destroy": (ip, [vp]),
        "svgf_reset": (ip, [vp]),
        "svgf_denoise": (ip, [vp, vp, vp, vp, cam, P(SvgfParams), vp]),
        "svgf_denoise_host": (ip, [vp, vp, vp, vp, cam, P(SvgfParams)]),
        "svgf_sync": (ip, [vp]),
        "svgf_last_error": (C.c_char_p, [vp]),
        "svgf_width": (ip, [vp]),
        "svgf_height": (ip, [vp]),
        "svgf_read_state": (ip, [vp, ip, vp, C.c_ulonglong]),
        "svgf_set_capture": (ip, [vp, ip]),
        "svgf_profile_enable": (ip, [vp, ip]),
        "svgf_profile_stride": (ip, [vp, ip]),
        "svgf_profile_frames": (C.c_longlong, [vp]),
        "svgf_profile_read": (ip, [vp, ip, ip, P(ip), fp, P(ip)]),
        "svgf_synth_camera": (ip, [ip, ip, ip, ip, cam, fp]),
        "svgf_synth_render": (ip, [ip, vp, vp, ip, ip, cam, synth, vp]),
        "svgf_scene_render": (ip, [ip, vp, vp, ip, ip, cam, synth, vp, ip, fp, vp]),
        "svgf_scene_render_mesh": (ip, [ip, vp, vp, ip, ip, cam, synth] + mesh + [fp, vp]),
        "svgf_display_pack": (ip, [ip, vp, vp, vp, ip, ip, vp]),
        "svgf_save_png": (ip, [C.c_char_p, vp, ip, ip, ip]),
        "svgf_planar_gbuffer": (ip, [vp, planes]),
        "svgf_denoise_planar": (ip, [vp, vp, vp, cam, P(SvgfParams), vp]),
        "svgf_synth_render_planar": (ip, [ip, vp, planes, ip, ip, cam, synth, vp]),
        "svgf_params_sizeof": (ip, None),
        "svgf_scene_render_mesh_planar": (ip, [ip, vp, planes, ip, ip, cam, synth] + mesh + [fp, vp]),
        "svgf_sync_stream": (ip, [vp, vp]),
        "svgf_build_has_experiments": (ip, None),
        "svgf_is_pipelined": (ip, [vp]),
        "svgf_create_ex": (ip, [ip, ip, ip, C.c_uint, P(vp)]),
        "svgf_enable_pipeline": (ip, [vp]),
        "svgf_pipeline_status": (ip, [vp]),
        "svgf_planar_gbuffer_stream": (ip, [vp, planes, vp]),
        "svgf_streams_overlap": (ip, [ip, vp, vp]),
        "svgf_denoise_motion": (ip, [vp, vp, vp, vp, vp, ip, cam, P(SvgfParams), vp]),
        "svgf_denoise_planar_motion": (ip, [vp, vp, vp, vp, ip, cam, P(SvgfParams), vp]),
        "svgf_motion_reproject": (ip, [ip, vp, ip, vp, vp, vp, ip, ip, cam, fp, vp, ip, vp]),
        "svgf_set_history_clamp": (ip, [vp, ip, fl]),
        "svgf_get_history_clamp": (ip, [vp, P(ip), fp]),
        "svgf_set_object_motion": (ip, [vp, vp, ip]),
        "svgf_get_object_motion": (ip, [vp, P(vp), P(ip)]),
        "svgf_set_firefly_filter": (ip, [vp, ip, fl]),
        "svgf_get_firefly_filter": (ip, [vp, P(ip), fp]),
        "svgf_set_output_taa": (ip, [vp, fl, fl]),
        "svgf_get_output_taa": (ip, [vp, fp, fp]),
        "svgf_upsample": (ip, [ip, vp, P(SvgfGuide), ip, ip, vp, P(SvgfGuide), ip, ip, P(SvgfUpsampleParams), vp]),
        "svgf_transfer_history": (ip, [vp, vp, vp]),
        "svgf_exposure_reset": (ip, [ip, vp, vp]),
        "svgf_exposure_meter": (ip, [ip, vp, vp, ip, ip, P(SvgfExposureParams), vp]),
        "svgf_display_tonemap": (ip, [ip, vp, vp, vp, ip, ip, P(SvgfTonemapParams), vp, vp]),
        "svgf_tonemap_srgb_table": (ip, [fp]),
        "svgf_quality_state_bytes": (C.c_ulonglong, [ip, ip]),
        "svgf_quality_windows": (ip, [ip, ip, P(ip), P(ip)]),
        "svgf_quality_meter": (ip, [ip, vp, vp, vp, ip, ip, P(SvgfQualityParams), vp, vp, vp, vp]),
        "svgf_quality_read": (ip, [ip, vp, P(SvgfQualityResult), vp]),
        "svgf_scene_create": (ip, [ip] + mesh + [P(SvgfSceneBuildParams), P(vp)]),
        "svgf_scene_destroy": (ip, [vp]),
        "svgf_scene_info": (ip, [vp, P(SvgfSceneInfo)]),
        "svgf_scene_draw": (ip, [vp, vp, vp, ip, ip, cam, synth, fp, vp]),
        "svgf_scene_draw_planar": (ip, [vp, vp, planes, ip, ip, cam, synth, fp, vp]),
        "svgf_bvh_build_host": (ip, [vp, ip, P(SvgfSceneBuildParams), vp, P(ip), vp, P(ip)]),
        "svgf_scene_enable_pose": (ip, [vp, ip]),
        "svgf_scene_pose": (ip, [vp, vp, ip, vp, vp]),
        "svgf_scene_read": (ip, [vp, ip, vp, C.c_ulonglong]),
        "svgf_pose_rigid": (ip, [fp, fl, fp, fp, vp]),
        "svgf_bvh_refit_plan_host": (ip, [vp, ip, ip, vp, vp, vp, vp, vp]),
        "svgf_scene_draw_shadowed": (ip, [vp, vp, vp, planes, ip, ip, cam, synth, P(SvgfSceneLight), vp]),
        "svgf_scene_view": (ip, [vp, P(SvgfSceneView)]),
        "svgf_scene_adopt_tree": (ip, [vp, vp, vp, ip, ip, ip]),
    }
    # what the experiments build (libsvgf_hip_exp.so) exports on top and the binding calls with arguments
    experiments = {
        "svgf_exp_set": (ip, [C.c_char_p, ip]),
        "svgf_exp_level_kernels": (ip, [vp, P(ip), P(ip), P(C.c_double), P(C.c_double), ip]),
        "svgf_exp_atrous_geometry": (ip, [ip] * 7 + [P(ip), P(C.c_double)]),
    }
    # every symbol include/svgf_lbvh.h declares
    lbvh = {
        "svgf_lbvh_create": (ip, [vp, P(SvgfLbvhParams), P(vp)]),
        "svgf_lbvh_build": (ip, [vp, vp]),
        "svgf_lbvh_attach": (ip, [vp, vp]),
        "svgf_lbvh_info": (ip, [vp, P(SvgfLbvhInfo)]),
        "svgf_lbvh_read": (ip, [vp, ip, vp, C.c_ulonglong]),
        "svgf_lbvh_destroy": (None, [vp]),
        "svgf_lbvh_version": (ip, None),
        "svgf_lbvh_build_host": (ip, [vp, ip, P(SvgfLbvhParams), vp, vp, vp, P(SvgfLbvhInfo)]),
    }
    return product, experiments, lbvh


_PROTOTYPES, _EXP_PROTOTYPES, _LBVH_PROTOTYPES = _prototypes()
EXPORTS, LBVH_EXPORTS = list(_PROTOTYPES), list(_LBVH_PROTOTYPES)


def _declare(lib, prototypes):
    for symbol, (restype, argtypes) in prototypes.items():
        f = getattr(lib, symbol)
        f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    return lib


_lib = None
_lib_exp = None
_default_experiments = False


def use_experiments_library(on: bool = True):
    """Tests / tools of parked experiments: make libsvgf_hip_exp.so the library every following Denoiser / producer call of this
    process uses (an explicit call — the binding reads no environment variable; the product path never calls this)."""
    global _default_experiments
    _default_experiments = bool(on)


def exp_set(name: str, value: int):
    """svgf_exp_set of the experiments build (process-wide; read by svgf_create / the launchers of libsvgf_hip_exp.so)."""
    _check(load_library(experiments=True).svgf_exp_set(name.encode(), int(value)), "svgf_exp_set", f"svgf_exp_set({name!r}, {value}) failed")


def exp_clear():
    load_library(experiments=True).svgf_exp_clear()


def atrous_geometry(kernel: str, W: int, H: int, step: int, blur_variance: int = 1, has_variance_plane: int = 1, n_cu: int = 256):
    """svgf_exp_atrous_geometry of the experiments build: ([supported, n_strips, seg_rows, n_segs, n_groups, grid blocks, block threads,
    LDS bytes], estimate in us or None) of one a-trous level on `kernel` (LEVEL_KERNEL_NAMES; lattice: [supported, log2k, pstride,
    band_rows, n_bands, grid blocks, block threads, LDS bytes]).  Host arithmetic only: works without a device."""
    out, est = (C.c_int * 8)(), C.c_double()
    rc = load_library(experiments=True).svgf_exp_atrous_geometry(LEVEL_KERNEL_NAMES.index(kernel), W, H, step, blur_variance, has_variance_plane,
                                                                 n_cu, out, C.byref(est))
    _check(rc, "svgf_exp_atrous_geometry", f"svgf_exp_atrous_geometry({kernel}, {W}x{H}, step {step}, {n_cu} CUs) -> {rc}")
    return list(out), (None if np.isnan(est.value) else est.value)


def load_library(path: str | None = None, experiments: bool = False):
    """Load libsvgf_hip.so (or, experiments=True / after use_experiments_library(), libsvgf_hip_exp.so) and declare prototypes.
    Fails loudly when the library is absent.  No environment variable is read."""
    global _lib, _lib_exp
    if path is None and not experiments and _default_experiments:
        experiments = True
    if path is None and experiments:
        if _lib_exp is None:
            _lib_exp = _declare(load_library(LIB_EXP_PATH), _EXP_PROTOTYPES)
        return _lib_exp
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.  If this library were loaded first it would bind the
    # system copy, and a process in which two HIP runtimes initialise can end up with one of them seeing no device.
    # Importing torch first (when it is installed) makes both share the copy torch already mapped.  torch is not
    # otherwise needed by the library.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(path):
        raise SvgfError(f"{path} not found: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                        "There is no CPU fallback.")
    lib = _declare(C.CDLL(path), _PROTOTYPES)
    if lib.svgf_params_sizeof() != C.sizeof(SvgfParams):     # the struct grows at its tail between ABI versions
        raise SvgfError(f"libsvgf_hip.so was built with sizeof(SvgfParams) = {lib.svgf_params_sizeof()}, this binding has {C.sizeof(SvgfParams)}")
    if path == LIB_PATH:
        _lib = lib
    return lib


def _draw_argtypes(params, table=False, split=False, virtual=False, rough=False, highlight=False):
    """The prototype of a companion draw from its parts: the scene, [the surface table], [direct, indirect], rgb, gbuffer, planes, width,
    height, camera, synth, light, the parameter block, [SvgfVirtualParams, chain], stream, [roughness table, SvgfRoughParams],
    [SvgfHighlightParams]."""
    vp, ip, P = C.c_void_p, C.c_int, C.POINTER
    return ([vp] + [vp] * table + [vp, vp] * split +
            [vp, vp, P(SvgfPlanarGBuffer), ip, ip, P(SvgfCamera), P(SvgfSynthParams), P(SvgfSceneLight), P(params)] +
            [P(SvgfVirtualParams), vp] * virtual + [vp] + [vp, P(SvgfRoughParams)] * rough + [P(SvgfHighlightParams)] * highlight)


# what the draws of a library take besides the common part (the split library draws with the trace library's)
_DRAW_PARTS = {"trace": dict(params=SvgfTraceParams), "path": dict(params=SvgfPathParams), "gloss": dict(params=SvgfPathParams, table=True),
               "virtual": dict(params=SvgfPathParams, table=True, virtual=True),
               "rough": dict(params=SvgfPathParams, table=True, virtual=True, rough=True),
               "highlight": dict(params=SvgfPathParams, table=True, virtual=True, rough=True, highlight=True)}
# the record a device table's create takes (svgf_<name>_table_create / _destroy / _size)
_TABLE_RECORD = {"gloss": SvgfSurface, "rough": C.c_float}


def _companion_prototypes(name):
    """The prototypes of libsvgf_<name>.so, a row of COMPANIONS, in _PROTOTYPES' form."""
    vp, ip, P = C.c_void_p, C.c_int, C.POINTER
    protos = {f"svgf_{name}_version": (ip, None)} if f"svgf_{name}_version" in companion_exports(name) else {}
    if name in _TABLE_RECORD:
        protos[f"svgf_{name}_table_create"] = (ip, [ip, P(_TABLE_RECORD[name]), ip, P(vp)])
        protos[f"svgf_{name}_table_destroy"] = (None, [vp])
        protos[f"svgf_{name}_table_size"] = (ip, [vp])
    if name == "split":
        protos["svgf_trace_draw_split"] = (ip, _draw_argtypes(split=True, **_DRAW_PARTS["trace"]))
        protos["svgf_trace_compose"] = (ip, [ip, vp, vp, vp, P(SvgfGuide), ip, ip, vp])
    else:
        protos[f"svgf_{name}_draw"] = (ip, _draw_argtypes(**_DRAW_PARTS[name]))
        if name != "trace":
            protos[f"svgf_{name}_draw_split"] = (ip, _draw_argtypes(split=True, **_DRAW_PARTS[name]))
    return protos


_linked_libs = {}


def _load_linked(name: str, prototypes):
    """Load libsvgf_<name>.so, a library that links against the product library (loaded first), declare prototypes(name) (a table in
    _PROTOTYPES' form) and keep the handle.  Fails loudly when the file is absent, and - where the table has svgf_<name>_version - when
    the library was compiled against another svgf.h than the product library found."""
    if name not in _linked_libs:
        product, path, table = load_library(), companion_path(name), prototypes(name)
        if not os.path.exists(path):
            raise SvgfError(f"{path} not found: build it first (python -c 'import __graft_entry__ as g; g.build()').")
        lib = _declare(C.CDLL(path), table)
        if f"svgf_{name}_version" in table:
            version = getattr(lib, f"svgf_{name}_version")
            if version() != product.svgf_version():
                raise SvgfError(f"libsvgf_{name}.so was built for ABI {version():#x}, libsvgf_hip.so is {product.svgf_version():#x}")
        _linked_libs[name] = lib
    return _linked_libs[name]


def _load_companion(name: str):
    return _load_linked(name, _companion_prototypes)


def _companion_loader(name):
    def load():
        return _load_companion(name)
    load.__name__ = load.__qualname__ = f"load_{name}_library"
    return load


(load_trace_library, load_split_library, load_path_library, load_gloss_library, load_virtual_library, load_rough_library,
 load_highlight_library) = (_companion_loader(c.name) for c in COMPANIONS)


def load_lbvh_library():
    """libsvgf_lbvh.so (row f24)."""
    return _load_linked("lbvh", lambda name: _LBVH_PROTOTYPES)


def lbvh_build_host(tri_boxes, leaf_tris: int = 0):
    """svgf_lbvh_build_host (no device needed): (nodes BVH_NODE_DTYPE[n_nodes], order int32[n_tris], keys uint64[n_tris], info dict) of
    the padded triangle boxes `tri_boxes` (BVH_NODE_DTYPE[n_tris]; lo and hi are read)."""
    tb = np.ascontiguousarray(tri_boxes, dtype=BVH_NODE_DTYPE)
    n = len(tb)
    L = int(leaf_tris) if 1 <= int(leaf_tris) <= 8 else 4
    nodes, order, keys = np.zeros(2 * max(-(-n // L), 1), BVH_NODE_DTYPE), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint64)
    info, p = SvgfLbvhInfo(), SvgfLbvhParams(int(leaf_tris))
    _call(load_lbvh_library(), "svgf_lbvh_build_host", tb.ctypes.data if n else None, n, C.byref(p), nodes.ctypes.data, order.ctypes.data,
          keys.ctypes.data, C.byref(info))
    return nodes[:info.n_nodes].copy(), order[:n].copy(), keys[:n].copy(), {k: int(getattr(info, k)) for k, _ in SvgfLbvhInfo._fields_}


class _DeviceTable:
    """One record per object id of a scene, on one device: allocated and uploaded once by svgf_<name>_table_create of libsvgf_<name>.so;
    usable as a context manager.  A subclass names the library and gives the records' numpy dtype and ctypes type."""
    name = record_dtype = record_ctype = None

    def __init__(self, records=None, device: int = 0):
        self.lib = _load_companion(self.name)
        arr = np.zeros(0, self.record_dtype) if records is None else np.ascontiguousarray(records, dtype=self.record_dtype).reshape(-1)
        self.h, h = C.c_void_p(), C.c_void_p()      # a table whose create failed stays without a handle
        _call(self.lib, f"svgf_{self.name}_table_create", int(device), arr.ctypes.data_as(C.POINTER(self.record_ctype)), len(arr), C.byref(h))
        self.h, self.device = h, int(device)

    def __len__(self):
        return int(getattr(self.lib, f"svgf_{self.name}_table_size")(self.h))

    def free(self):
        if self.h:
            getattr(self.lib, f"svgf_{self.name}_table_destroy")(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RoughTable(_DeviceTable):
    """svgf_rough_table: the GGX roughness of a scene's objects on one device, one float32 per object id, 0 = smooth.  `alpha` is
    anything np.asarray turns into float32 (None or empty: a table of no entries).  Allocates and uploads once; usable as a context
    manager."""
    name, record_dtype, record_ctype = "rough", np.float32, C.c_float

    def __init__(self, alpha=None, device: int = 0):
        super().__init__(alpha, device)


class GlossTable(_DeviceTable):
    """svgf_gloss_table: the surfaces of a scene's objects on one device, one SvgfSurface per object id.  `surfaces` is a numpy array
    of scene.SURFACE_DTYPE (or anything np.asarray turns into one; None or empty: a table of no records).  Allocates and uploads once;
    usable as a context manager."""
    name, record_ctype = "gloss", SvgfSurface

    def __init__(self, surfaces=None, device: int = 0):
        from . import scene as _scene
        self.record_dtype = _scene.SURFACE_DTYPE
        super().__init__(surfaces, device)


# int or float per field of the companions' parameter blocks
_CONVERTERS = {s: tuple(float if t is C.c_float else int for _, t in s._fields_)
               for s in (SvgfTraceParams, SvgfPathParams, SvgfVirtualParams, SvgfRoughParams, SvgfHighlightParams)}


def _filled(struct, values):
    """`struct` with its fields set from `values`, each converted to its field's type."""
    return struct(*[c(v) for c, v in zip(_CONVERTERS[struct], values)])


class Denoiser:
    """One SVGF context on one GPU (denoiseInit .. denoiseFree of the reference, handle-based)."""

    def __init__(self, width: int, height: int, device: int = 0, experiments: bool = False, pipelined: bool = False):
        """pipelined=True: svgf_create_ex(SVGF_CREATE_PIPELINED) — the frame pipeline's resources exist from the start
        (SvgfParams.inputs_ready is ignored by any other context).
        experiments=True: the context lives in libsvgf_hip_exp.so (kernel_variant 5 / 6, exp_set knobs) — tests and tools only."""
        self.lib = load_library(experiments=experiments)
        self.width, self.height = int(width), int(height)
        self.device = int(device)
        self.ui = SvgfParams()
        self.lib.svgf_params_default(C.byref(self.ui))
        self.h, h = None, C.c_void_p()      # no context yet: a failing create reports the library's own last error
        self._check(self.lib.svgf_create_ex(int(device), self.width, self.height, CREATE_PIPELINED if pipelined else 0, C.byref(h)),
                    f"svgf_create_ex({device},{width},{height})")
        self.h = h

    def _check(self, rc, what):
        if rc != SVGF_OK:
            raise SvgfError(f"{what} -> {rc}: {self.lib.svgf_last_error(self.h).decode()}")

    def _frame(self, camera, params, stream=None):
        """What every denoise entry point takes last: the camera and the parameter block (`params` or self.ui) by reference, the stream."""
        return C.byref(_camera(camera)), C.byref(params if params is not None else self.ui), _stream(stream)

    def _pair(self, symbol, first, second):
        """A getter with two out-parameters."""
        self._check(getattr(self.lib, symbol)(self.h, C.byref(first), C.byref(second)), symbol)
        return first.value, second.value

    # --- reference-named lifecycle ---
    def free(self):
        if getattr(self, "h", None):
            self.lib.svgf_destroy(self.h)
            self.h = None

    denoiseFree = free

    def reset(self):
        self._check(self.lib.svgf_reset(self.h), "svgf_reset")

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def denoise(self, out, inp, gbuffer, camera, params: SvgfParams | None = None, stream=None, motion=None,
                motion_format: int = MOTION_PREV_COORD_F32):
        """Device pointers (ints) or contiguous CUDA torch tensors.  Asynchronous on `stream`.
        motion: a device plane of per-pixel previous-frame coordinates in `motion_format` (svgf_denoise_motion); None: the
        history is found through the previous camera (svgf_denoise)."""
        frame = self._frame(camera, params, stream)
        if motion is None:
            self._check(self.lib.svgf_denoise(self.h, _ptr(out), _ptr(inp), _ptr(gbuffer), *frame), "svgf_denoise")
        else:
            self._check(self.lib.svgf_denoise_motion(self.h, _ptr(out), _ptr(inp), _ptr(gbuffer), _ptr(motion), int(motion_format), *frame),
                        "svgf_denoise_motion")

    def planar_gbuffer(self, stream=None) -> SvgfPlanarGBuffer:
        """The planes the NEXT denoise_planar() call consumes: a producer fills them in place.
        stream given: svgf_planar_gbuffer_stream — on a pipelined context the producer's stream waits for exactly the frames that
        still read those planes instead of the host waiting for the device."""
        g = SvgfPlanarGBuffer()
        if stream is None:
            self._check(self.lib.svgf_planar_gbuffer(self.h, C.byref(g)), "svgf_planar_gbuffer")
        else:
            self._check(self.lib.svgf_planar_gbuffer_stream(self.h, C.byref(g), _stream(stream)), "svgf_planar_gbuffer_stream")
        return g

    def denoise_planar(self, out, inp, camera, params: SvgfParams | None = None, stream=None, motion=None,
                       motion_format: int = MOTION_PREV_COORD_F32):
        """One frame whose G-buffer was written into planar_gbuffer()'s planes.  Asynchronous on `stream`.  motion: as in denoise()."""
        frame = self._frame(camera, params, stream)
        if motion is None:
            self._check(self.lib.svgf_denoise_planar(self.h, _ptr(out), _ptr(inp), *frame), "svgf_denoise_planar")
        else:
            self._check(self.lib.svgf_denoise_planar_motion(self.h, _ptr(out), _ptr(inp), _ptr(motion), int(motion_format), *frame),
                        "svgf_denoise_planar_motion")

    def denoise_host(self, color: np.ndarray, gbuffer: np.ndarray, camera, params: SvgfParams | None = None, motion=None,
                     motion_format: int = MOTION_PREV_COORD_F32) -> np.ndarray:
        """numpy in, numpy out (uploads, runs, downloads, synchronises).  motion: a HOST array of H*W previous-frame coordinates
        in `motion_format` (float32[H, W, 2], or float16[H, W, 2] for MOTION_DELTA_F16); it is uploaded with torch."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        gbuffer = np.ascontiguousarray(gbuffer)
        assert color.size == 3 * self.width * self.height and gbuffer.nbytes == 52 * self.width * self.height
        out = np.empty_like(color)
        if motion is None:
            self._check(self.lib.svgf_denoise_host(self.h, out.ctypes.data, color.ctypes.data, gbuffer.ctypes.data,
                                                   *self._frame(camera, params)[:2]), "svgf_denoise_host")
            return out
        import torch
        motion = np.ascontiguousarray(motion, dtype=np.float16 if motion_format == MOTION_DELTA_F16 else np.float32)
        assert motion.size == 2 * self.width * self.height
        dev = torch.device("cuda", self.device)
        t_in = torch.from_numpy(color).to(dev)
        t_g = torch.from_numpy(gbuffer.view(np.uint8).reshape(-1)).to(dev)
        t_m = torch.from_numpy(motion).to(dev)
        t_out = torch.empty(color.shape, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self.denoise(t_out, t_in, t_g, camera, params, motion=t_m, motion_format=motion_format)
        self.sync()
        return t_out.cpu().numpy()

    def sync(self):
        self._check(self.lib.svgf_sync(self.h), "svgf_sync")

    def is_pipelined(self) -> bool:
        """True while the context's frames alternate between its two plane sets (include/svgf.h: svgf_is_pipelined)."""
        return bool(self.lib.svgf_is_pipelined(self.h))

    def enable_pipeline(self):
        """svgf_enable_pipeline: create the frame pipeline's resources now (allocates, synchronises the device, probes the queues)."""
        self._check(self.lib.svgf_enable_pipeline(self.h), "svgf_enable_pipeline")

    def pipeline_status(self) -> int:
        """0 no resources, 1 promise honoured, 2 promise refused (internal streams share a hardware queue)."""
        return int(self.lib.svgf_pipeline_status(self.h))

    def last_error(self) -> str:
        return self.lib.svgf_last_error(self.h).decode()

    def sync_stream(self, stream=None):
        """Wait for what has been enqueued on `stream` only (svgf_sync waits for the whole device, as the reference does)."""
        self._check(self.lib.svgf_sync_stream(self.h, _stream(stream)), "svgf_sync_stream")

    def level_kernels(self) -> list[tuple[str, int, float | None, float | None]]:
        """Experiments build only: per a-trous level of the last frame, (kernel name, step, lane estimate us, strip estimate us);
        the estimates are None where the automatic lane / strip choice was not consulted.  Kernel names: LEVEL_KERNEL_NAMES."""
        if not hasattr(self.lib, "svgf_exp_level_kernels"):
            raise SvgfError("level_kernels: this context is not in the experiments build (Denoiser(..., experiments=True))")
        kinds, steps = (C.c_int * MAX_LEVELS)(), (C.c_int * MAX_LEVELS)()
        lane, strip = (C.c_double * MAX_LEVELS)(), (C.c_double * MAX_LEVELS)()
        n = self.lib.svgf_exp_level_kernels(self.h, kinds, steps, lane, strip, MAX_LEVELS)
        if n < 0:
            raise SvgfError(f"svgf_exp_level_kernels -> {n}")
        est = lambda v: None if np.isnan(v) else float(v)      # noqa: E731
        return [(LEVEL_KERNEL_NAMES[kinds[k]], int(steps[k]), est(lane[k]), est(strip[k])) for k in range(n)]

    def set_capture(self, on: bool = True):
        self._check(self.lib.svgf_set_capture(self.h, 1 if on else 0), "svgf_set_capture")

    def set_history_clamp(self, radius: int, sigma_scale: float = 1.0):
        """svgf_set_history_clamp: clamp the reprojected history colour to mean +- sigma_scale * sigma of the current frame's
        (2 radius + 1)^2 colour window before the blend; radius 0 (the default) = off, 1..3.  Survives reset()."""
        self._check(self.lib.svgf_set_history_clamp(self.h, int(radius), float(sigma_scale)), "svgf_set_history_clamp")

    def history_clamp(self) -> tuple[int, float]:
        """(radius, sigma_scale) as set by set_history_clamp(); (0, 0.0) on a fresh context."""
        return self._pair("svgf_get_history_clamp", C.c_int(), C.c_float())

    def set_firefly_filter(self, rank: int, scale: float = 1.0):
        """svgf_set_firefly_filter: frames run as if the input colour had been filtered, every pixel brighter than scale times the
        rank-th largest luminance of its 8 neighbours scaled down to that bound; rank 0 (the default) = off, 1..3.  Survives reset()."""
        self._check(self.lib.svgf_set_firefly_filter(self.h, int(rank), float(scale)), "svgf_set_firefly_filter")

    def firefly_filter(self) -> tuple[int, float]:
        """(rank, scale) as set by set_firefly_filter(); (0, 0.0) on a fresh context."""
        return self._pair("svgf_get_firefly_filter", C.c_int(), C.c_float())

    def set_output_taa(self, alpha: float, sigma_scale: float = 1.0):
        """svgf_set_output_taa: blend every frame's image with the previous frame's output, reprojected like the temporal pass's
        history and clipped to mean +- sigma_scale * sigma of the image's 3x3 window: out = alpha * image + (1 - alpha) * history.
        alpha 0 (the default) = off, else 0 < alpha <= 1.  The first call that turns it on allocates 44 B/px and may synchronise
        the device.  Survives reset() (the output history does not)."""
        self._check(self.lib.svgf_set_output_taa(self.h, float(alpha), float(sigma_scale)), "svgf_set_output_taa")

    def output_taa(self) -> tuple[float, float]:
        """(alpha, sigma_scale) as set by set_output_taa(); (0.0, 0.0) on a fresh context."""
        return self._pair("svgf_get_output_taa", C.c_float(), C.c_float())

    def set_object_motion(self, geom_xf, n_geoms: int | None = None):
        """svgf_set_object_motion: geom_xf is a contiguous device float32[n, 12] tensor (or a raw pointer with n_geoms) of 3x4
        row-major maps, this frame's world space -> the previous frame's, indexed by geomId; None = off.  The temporal pass tests
        a tap's history against the pixel's normal and position moved by its object's map, and without a motion plane looks the
        history up where the moved position projects.  The context keeps the POINTER: the tensor must stay alive, and is
        refreshed in place on the frame's stream before each frame.  Survives reset()."""
        if n_geoms is None:
            n_geoms = 0 if geom_xf is None else int(geom_xf.numel()) // 12
        self._check(self.lib.svgf_set_object_motion(self.h, _ptr(geom_xf), int(n_geoms)), "svgf_set_object_motion")

    def object_motion(self) -> tuple[int | None, int]:
        """(device pointer or None, n_geoms) as set by set_object_motion(); (None, 0) on a fresh context."""
        return self._pair("svgf_get_object_motion", C.c_void_p(), C.c_int())

    def transfer_history_from(self, src: "Denoiser", stream=None):
        """svgf_transfer_history: everything this context's next frame reads as history becomes `src`'s, resampled to this
        context's size (colour history, moments, history lengths, previous G-buffer planes, previous view, and the output history
        when both contexts have one); at equal sizes a bit-exact clone.  One launch on `stream`; this context's settings stay,
        `src` is only read.  Both contexts' unfinished frames must have been given to `stream`, and this context's next frame
        goes there too."""
        if not isinstance(src, Denoiser) or src.lib is not self.lib:
            raise SvgfError("transfer_history_from: src must be a Denoiser of the same library")
        self._check(self.lib.svgf_transfer_history(self.h, src.h, _stream(stream)), "svgf_transfer_history")

    def read_state(self, which: int) -> np.ndarray:
        """Host copy of one state plane (STATE_*); STATE_OUTPUT_HISTORY is float32[H, W, 4] = {r, g, b, geomId bits} and raises
        while the context has no output history."""
        n = self.width * self.height
        shape, dt = {STATE_HISTORY_LENGTH: ((self.height, self.width), np.int32),
                     STATE_MOMENTS: ((self.height, self.width, 2), np.float32),
                     STATE_COLOR_HISTORY: ((self.height, self.width, 3), np.float32),
                     STATE_VARIANCE_TEMPORAL: ((self.height, self.width), np.float32),
                     STATE_COLOR_ACC: ((self.height, self.width, 3), np.float32),
                     STATE_PREV_NORMAL: ((self.height, self.width, 3), np.float32),
                     STATE_PREV_POSITION: ((self.height, self.width, 3), np.float32),
                     STATE_PREV_GEOM_ID: ((self.height, self.width), np.int32),
                     STATE_OUTPUT_HISTORY: ((self.height, self.width, 4), np.float32)}[which]
        a = np.empty(shape, dtype=dt)
        assert a.size >= n
        self._check(self.lib.svgf_read_state(self.h, which, a.ctypes.data, a.nbytes), "svgf_read_state")
        return a

    # --- profiling ---
    def profile_enable(self, nframes: int):
        self._check(self.lib.svgf_profile_enable(self.h, int(nframes)), "svgf_profile_enable")

    def profile_stride(self, k: int):
        self._check(self.lib.svgf_profile_stride(self.h, int(k)), "svgf_profile_stride")

    def profile_frames(self) -> int:
        return int(self.lib.svgf_profile_frames(self.h))

    def profile_read(self, slot: int):
        kinds = (C.c_int * 32)()
        ms = (C.c_float * 32)()
        n = C.c_int()
        self._check(self.lib.svgf_profile_read(self.h, slot, 32, kinds, ms, C.byref(n)), "svgf_profile_read")
        return [(kinds[i], ms[i]) for i in range(n.value)]


# --- the denoiser's inputs produced on the device -------------------------------------------
def streams_overlap(stream_a, stream_b, device: int = 0) -> bool:
    """svgf_streams_overlap: do kernels on the caller's two streams run side by side (what inputs_ready = 2 needs)?"""
    rc = load_library().svgf_streams_overlap(int(device), _stream(stream_a), _stream(stream_b))
    if rc < 0:
        raise SvgfError(f"svgf_streams_overlap failed ({rc})")
    return bool(rc)


def synth_camera(frame: int, moving: bool, width: int, height: int):
    """svgf_synth_camera: (SvgfCamera, (plx, ply)) computed by the library (C float math)."""
    cam = SvgfCamera()
    pl = (C.c_float * 2)()
    _call(load_library(), "svgf_synth_camera", int(frame), int(bool(moving)), int(width), int(height), C.byref(cam), pl)
    return cam, (pl[0], pl[1])


def synth_render(out_rgb, out_gbuffer, width: int, height: int, camera, frame: int, seed: int = 1,
                 noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, device: int = 0, stream=None):
    """svgf_synth_render: writes packed rgb (H*W*3 float32) and 52-byte texels (H*W*52 bytes) into device memory
    (torch CUDA tensors or raw pointers).  `camera` is an SvgfCamera or a synth.camera_for_frame() dict;
    `pixel_length` defaults to synth._pixel_length(width, height, 45) so that host and device producers agree."""
    cam, sp = _view(camera, width, height, frame, seed, noise, fireflies, pixel_length, camera_fovy=False)
    _call(load_library(), "svgf_synth_render", int(device), _ptr(out_rgb), _ptr(out_gbuffer), int(width), int(height), C.byref(cam), C.byref(sp),
          _stream(stream))


def synth_render_planar(out_rgb, planes: SvgfPlanarGBuffer, width: int, height: int, camera, frame: int, seed: int = 1,
                        noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, device: int = 0, stream=None):
    """svgf_synth_render_planar: the frame of synth_render written into a Denoiser's planar_gbuffer() planes."""
    cam, sp = _view(camera, width, height, frame, seed, noise, fireflies, pixel_length, camera_fovy=False)
    _call(load_library(), "svgf_synth_render_planar", int(device), _ptr(out_rgb), C.byref(planes), int(width), int(height), C.byref(cam),
          C.byref(sp), _stream(stream))


# --- per-pixel motion vectors: the plane svgf_denoise_motion reads, for rigid motion --------------------------------------
def motion_reproject(motion_out, width: int, height: int, prev_camera, gbuffer=None, position=None, geom_id=None,
                     motion_format: int = MOTION_PREV_COORD_F32, reproj_scale=(0.0, 0.0), geom_xf=None, n_geoms: int | None = None,
                     device: int = 0, stream=None):
    """svgf_motion_reproject: per pixel the previous-frame coordinate of the texel's position (AoS `gbuffer`, or the `position` /
    `geom_id` planes — tensors, raw pointers or a SvgfPlanarGBuffer's fields), mapped by geom_xf[geomId] (device float32[n, 12], 3x4
    row-major, this frame's world -> the previous frame's) and projected through `prev_camera` exactly as the temporal pass does.
    `motion_out`: device memory of width * height * 2 float32 (float16 for MOTION_DELTA_F16)."""
    rs = (C.c_float * 2)(float(reproj_scale[0]), float(reproj_scale[1]))
    if geom_xf is not None and n_geoms is None:
        n_geoms = int(geom_xf.numel()) // 12
    _call(load_library(), "svgf_motion_reproject", int(device), _ptr(motion_out), int(motion_format), _ptr(gbuffer), _ptr(position), _ptr(geom_id),
          int(width), int(height), C.byref(_camera(prev_camera)), rs, _ptr(geom_xf), int(n_geoms or 0), _stream(stream))


# --- guided upsampling: the full-size image from a reduced-size denoise ----------------------------------------------------
def guide(gbuffer=None, normal=None, position=None, geom_id=None, albedo=None) -> SvgfGuide:
    """A SvgfGuide from AoS texels (`gbuffer`) or planes: tensors, raw pointers or a SvgfPlanarGBuffer's fields."""
    return SvgfGuide(_ptr(gbuffer), _ptr(normal), _ptr(position), _ptr(geom_id), _ptr(albedo))


def upsample(out, hi_guide, width_hi: int, height_hi: int, rgb_lo, lo_guide, width_lo: int, height_lo: int,
             sigma_n: float, sigma_x: float, modulate, device: int = 0, stream=None):
    """svgf_upsample: `out` (device, height_hi * width_hi * 3 float32) from `rgb_lo`, the output of a denoise at width_lo x height_lo
    run with sepcolor = 1 and addcolor = 0, guided by the two G-buffers.  A guide is a SvgfGuide (guide(...)) or the AoS texels
    themselves (a tensor or a raw pointer).  sigma_x is in the scene's world units; 0 turns a term off."""
    hi, lo = (g if isinstance(g, SvgfGuide) else guide(gbuffer=g) for g in (hi_guide, lo_guide))
    up = SvgfUpsampleParams(float(sigma_n), float(sigma_x), int(modulate))
    _call(load_library(), "svgf_upsample", int(device), _ptr(out), C.byref(hi), int(width_hi), int(height_hi), _ptr(rgb_lo), C.byref(lo),
          int(width_lo), int(height_lo), C.byref(up), _stream(stream))


def trace_compose(out, direct, indirect, guide_or_gbuffer, width: int, height: int, device: int = 0, stream=None):
    """svgf_trace_compose of libsvgf_split.so (row f18): out = albedo * (direct + indirect), the albedo from a SvgfGuide (guide(...):
    AoS texels, or an albedo plane) or from the AoS texels themselves (a tensor or a raw pointer).  `out` may be `direct` or
    `indirect`.  One launch on `stream`; never waits."""
    g = guide_or_gbuffer if isinstance(guide_or_gbuffer, SvgfGuide) else guide(gbuffer=guide_or_gbuffer)
    _call(load_split_library(), "svgf_trace_compose", int(device), _ptr(out), _ptr(direct), _ptr(indirect), C.byref(g), int(width), int(height),
          _stream(stream))


# --- the step after denoise() ----------------------------------------------------------------
def display_pack(pbo, left, right, width: int, height: int, device: int = 0, stream=None):
    """svgf_display_pack: `left` | `right` (packed rgb float, device) -> (height, 2*width, 4) uint8 in device memory."""
    _call(load_library(), "svgf_display_pack", int(device), _ptr(pbo), _ptr(left), _ptr(right), int(width), int(height), _stream(stream))


# --- row f12: HDR display (luminance histogram, auto-exposure, tone-mapped pack) ---------------------------------------------------
def exposure_reset(state, device: int = 0, stream=None):
    """svgf_exposure_reset: `state` (device, EXPOSURE_STATE_WORDS int32) back to "no metering yet", exposure 1."""
    _call(load_library(), "svgf_exposure_reset", int(device), _ptr(state), _stream(stream))


def exposure_state(device: int = 0):
    """A fresh exposure state on `device`: a 520-element int32 tensor, already reset (the reset has completed on return)."""
    import torch
    state = torch.empty((EXPOSURE_STATE_WORDS,), dtype=torch.int32, device=f"cuda:{int(device)}")
    exposure_reset(state, device=device)
    torch.cuda.synchronize(int(device))
    return state


def exposure_meter(state, rgb, width: int, height: int, key: float = 0.18, trim_low_1024: int = 51, trim_high_1024: int = 51,
                   min_exposure: float = 1.0 / 64.0, max_exposure: float = 64.0, adapt: float = 1.0, device: int = 0, stream=None):
    """svgf_exposure_meter: the luminance histogram of `rgb` (packed rgb float, device) and the exposure step, into `state`."""
    ep = SvgfExposureParams(float(key), int(trim_low_1024), int(trim_high_1024), float(min_exposure), float(max_exposure), float(adapt))
    _call(load_library(), "svgf_exposure_meter", int(device), _ptr(state), _ptr(rgb), int(width), int(height), C.byref(ep), _stream(stream))


def display_tonemap(pbo, left, right, width: int, height: int, op: int = TONEMAP_ACES, transfer: int = TRANSFER_SRGB,
                    exposure_bias: float = 1.0, white: float = 0.0, state=None, device: int = 0, stream=None):
    """svgf_display_tonemap: `left` | `right` (or `right` alone when `left` is None) through exposure (exposure_bias x the metered
    exposure of `state`, or exposure_bias alone), tone curve and display transfer -> (height, 2*width or width, 4) uint8 on the device."""
    tp = SvgfTonemapParams(int(op), int(transfer), float(exposure_bias), float(white))
    _call(load_library(), "svgf_display_tonemap", int(device), _ptr(pbo), _ptr(left), _ptr(right), int(width), int(height), C.byref(tp),
          _ptr(state), _stream(stream))


def srgb_table() -> np.ndarray:
    """svgf_tonemap_srgb_table: the 256 float32 thresholds transfer 2 searches."""
    t = np.empty(256, dtype=np.float32)
    _call(load_library(), "svgf_tonemap_srgb_table", t.ctypes.data_as(C.POINTER(C.c_float)))
    return t


# --- row f13: image-quality meter (MSE / PSNR, largest error, windowed SSIM of two device images) ----------------------------------
def quality_windows(width: int, height: int):
    """svgf_quality_windows: (nwx, nwy), the 8 x 8 windows at stride 4 that fit; (0, 0) below 8 pixels either way."""
    nwx, nwy = C.c_int(), C.c_int()
    _call(load_library(), "svgf_quality_windows", int(width), int(height), C.byref(nwx), C.byref(nwy))
    return nwx.value, nwy.value


def quality_state(width: int, height: int, device: int = 0):
    """The meter's state for a width x height comparison on `device`: svgf_quality_state_bytes bytes as an int64 tensor (the first
    eight words are the result block), deliberately NOT zeroed: svgf_quality_meter rewrites everything it later reads."""
    import torch
    n = int(load_library().svgf_quality_state_bytes(int(width), int(height)))
    if n == 0:
        raise SvgfError(f"svgf_quality_state_bytes({width}, {height}) = 0: a size <= 0 or an unsupported one")
    return torch.empty((n // 8,), dtype=torch.int64, device=f"cuda:{int(device)}")


def quality_meter(state, a, b, width: int, height: int, peak: float = 1.0, scale: float = 1.0, clamp: int = 0, exposure_state=None,
                  se_map=None, ssim_map=None, device: int = 0, stream=None):
    """svgf_quality_meter: `a` (under test) against `b` (the reference), packed rgb float on the device, into `state`
    (quality_state); `exposure_state` is f12's state (the effective scale is scale x its exposure); the maps are optional device
    float32 outputs of height x width and quality_windows' nwy x nwx elements."""
    qp = SvgfQualityParams(float(peak), float(scale), int(clamp))
    _call(load_library(), "svgf_quality_meter", int(device), _ptr(state), _ptr(a), _ptr(b), int(width), int(height), C.byref(qp),
          _ptr(exposure_state), _ptr(se_map), _ptr(ssim_map), _stream(stream))


def quality_read(state, device: int = 0, stream=None) -> dict:
    """svgf_quality_read: waits for `stream` and returns the result block and mse / psnr_db / mean_ssim as a dict."""
    r = SvgfQualityResult()
    _call(load_library(), "svgf_quality_read", int(device), _ptr(state), C.byref(r), _stream(stream))
    return {n: getattr(r, n) for n, _ in SvgfQualityResult._fields_}


def save_png(path: str, rgb: np.ndarray, mirror_x: bool = True):
    """svgf_save_png: host float32 (H, W, 3) -> 8-bit RGB PNG, with the reference's x mirror by default."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[0], rgb.shape[1]
    _call(load_library(), "svgf_save_png", os.fsencode(path), rgb.ctypes.data, int(w), int(h), int(bool(mirror_x)))


# --- scene-driven producer -------------------------------------------------------------------
def _scene_arrays(geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures):
    """The host arrays svgf_scene_render_mesh / svgf_scene_create take, as (arrays to keep alive, ctypes arguments)."""
    from . import scene as _scene
    geoms = np.zeros(0, _scene.SCENE_GEOM_DTYPE) if geoms is None else np.ascontiguousarray(geoms, dtype=_scene.SCENE_GEOM_DTYPE)
    gi = np.ascontiguousarray(geom_ids if geom_ids is not None else np.zeros(0, np.int32), dtype=np.int32)
    tr = np.ascontiguousarray(tris if tris is not None else np.zeros((0, 24), np.float32), dtype=np.float32).reshape(-1, 24)
    ti = np.ascontiguousarray(tri_ids if tri_ids is not None else np.zeros(0, np.int32), dtype=np.int32)
    ta = np.ascontiguousarray(tri_albedo if tri_albedo is not None else np.zeros((0, 3), np.float32), dtype=np.float32).reshape(-1, 3)
    n_tex, tt, td, tx = 0, None, None, None
    if textures is not None and len(textures) and tri_tex is not None:      # list of uint8[h, w, 3]; tri_tex: index per triangle, -1 = none
        n_tex = len(textures)
        tt = np.ascontiguousarray(tri_tex, dtype=np.int32)
        blobs = [np.ascontiguousarray(t, dtype=np.uint8) for t in textures]
        offs = np.cumsum([0] + [b.size for b in blobs[:-1]])
        td = np.array([[o, b.shape[1], b.shape[0]] for o, b in zip(offs, blobs)], dtype=np.int32)
        tx = np.concatenate([b.reshape(-1) for b in blobs])
    ptr = lambda a, on=True: a.ctypes.data if (a is not None and on and a.size) else None       # noqa: E731
    args = (ptr(geoms), int(len(geoms)), ptr(gi), ptr(tr), ptr(ti), ptr(ta), int(len(tr)), ptr(tt, n_tex), ptr(td, n_tex), ptr(tx, n_tex), int(n_tex))
    return (geoms, gi, tr, ti, ta, tt, td, tx), args


def _light_of(geoms, light):
    from . import scene as _scene
    return _v3(_scene.light_position(geoms) if light is None else np.asarray(light, dtype=np.float32))


def scene_render(out_rgb, out_gbuffer, width: int, height: int, camera, geoms: np.ndarray, frame: int, seed: int = 1,
                 noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, light=None, device: int = 0, stream=None):
    """svgf_scene_render: `geoms` is a scene.SCENE_GEOM_DTYPE array (scene.geom_array(scene.parse_scene(text)))."""
    from . import scene as _scene
    cam, sp = _view(camera, width, height, frame, seed, noise, fireflies, pixel_length, camera_fovy=True)
    geoms = np.ascontiguousarray(geoms, dtype=_scene.SCENE_GEOM_DTYPE)
    _call(load_library(), "svgf_scene_render", int(device), _ptr(out_rgb), _ptr(out_gbuffer), int(width), int(height), C.byref(cam), C.byref(sp),
          geoms.ctypes.data, int(len(geoms)), _light_of(geoms, light), _stream(stream))


def scene_render_mesh(out_rgb, out_gbuffer, width: int, height: int, camera, geoms: np.ndarray, geom_ids, tris, tri_ids, tri_albedo,
                      frame: int, tri_tex=None, textures=None, seed: int = 1, noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, light=None,
                      device: int = 0, stream=None):
    """svgf_scene_render_mesh: primitives (`geoms`, geomId = geom_ids[k]) + world-space triangles (`tris` float32[n,3,8] =
    pos, normal, uv per corner; geomId = tri_ids[i]; albedo = tri_albedo[i]).  The library has read the host arrays completely
    when it returns (it waits for its uploads); the kernel itself stays asynchronous on `stream`.
    `out_gbuffer` may be a SvgfPlanarGBuffer (Denoiser.planar_gbuffer()): svgf_scene_render_mesh_planar writes the planes."""
    cam, sp = _view(camera, width, height, frame, seed, noise, fireflies, pixel_length, camera_fovy=True)
    keep, args = _scene_arrays(geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures)
    planar, texels, planes = _draw_target(out_gbuffer)
    rc = getattr(load_library(), "svgf_scene_render_mesh_planar" if planar else "svgf_scene_render_mesh")(
        int(device), _ptr(out_rgb), planes if planar else texels, int(width), int(height), C.byref(cam), C.byref(sp), *args,
        _light_of(keep[0], light), _stream(stream))
    _check(rc, "svgf_scene_render_mesh")
    if stream is None:
        import torch
        torch.cuda.synchronize(int(device))


# --- row f14: resident scene (upload once, BVH over the triangles, one launch per frame) ------------------------------------------
def bvh_build_host(tris, max_leaf_tris: int = 0, split: int = 0):
    """svgf_bvh_build_host (no device needed): (nodes BVH_NODE_DTYPE[n_nodes], order int32[n_tris], depth) of `tris`
    (float32[n, 3, 8] or [n, 24])."""
    tr = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 24)
    n = len(tr)
    nodes, order = np.zeros(2 * max(n, 1), BVH_NODE_DTYPE), np.zeros(max(n, 1), np.int32)
    n_nodes, depth = C.c_int(-1), C.c_int(-1)
    bp = SvgfSceneBuildParams(int(max_leaf_tris), int(split))
    _call(load_library(), "svgf_bvh_build_host", tr.ctypes.data if n else None, n, C.byref(bp), nodes.ctypes.data, C.byref(n_nodes),
          order.ctypes.data, C.byref(depth))
    return nodes[:n_nodes.value].copy(), order[:n].copy(), depth.value


def pose_rigid(axis, angle_rad: float, pivot=(0.0, 0.0, 0.0), translate=(0.0, 0.0, 0.0)) -> np.ndarray:
    """svgf_pose_rigid (host only): one SCENE_POSE_DTYPE record - the rotation by angle_rad about `axis` through `pivot`, then
    `translate`, and its analytic inverse."""
    out = np.zeros(1, SCENE_POSE_DTYPE)
    _call(load_library(), "svgf_pose_rigid", _v3(axis), float(angle_rad), _v3(pivot), _v3(translate), out.ctypes.data)
    return out[0]


def pose_identity(n: int) -> np.ndarray:
    """n identity SCENE_POSE_DTYPE records."""
    out = np.zeros(int(n), SCENE_POSE_DTYPE)
    out["xf"][:, [0, 5, 10]] = 1.0
    out["inv"][:, [0, 5, 10]] = 1.0
    return out


def bvh_refit_plan_host(nodes, cap: int = SCENE_REFIT_CAP) -> dict:
    """svgf_bvh_refit_plan_host (no device needed): dict(treelets REFIT_TREELET_DTYPE[n_treelets], level uint8[n_nodes],
    top int32[n_top], top_seg int32[n_top_depths + 1]) of BVH_NODE_DTYPE `nodes`."""
    nd = np.ascontiguousarray(nodes, dtype=BVH_NODE_DTYPE)
    n = len(nd)
    treelets, level, top = np.zeros(max(n, 1), REFIT_TREELET_DTYPE), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32)
    seg, info = np.zeros(SCENE_MAX_DEPTH + 2, np.int32), np.zeros(4, np.int32)
    _call(load_library(), "svgf_bvh_refit_plan_host", nd.ctypes.data if n else None, n, int(cap), treelets.ctypes.data, level.ctypes.data,
          top.ctypes.data, seg.ctypes.data, info.ctypes.data)
    return dict(treelets=treelets[:info[0]].copy(), level=level[:n].copy(), top=top[:info[1]].copy(), top_seg=seg[:info[2] + 1].copy())


class Scene:
    """A resident scene: svgf_scene_create once (validates, builds the BVH, uploads; allocates and synchronises), then draw() /
    draw_planar() per frame - one launch each on `stream`, nothing else.  Camera, light and noise change per draw; with
    enable_pose(n) once and pose(table) per frame (row f15) the objects move rigidly too.  Topology and textures are fixed."""

    def __init__(self, handle, device):
        self.lib, self.h, self.device = load_library(), handle, int(device)

    @classmethod
    def create(cls, geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex=None, textures=None, max_leaf_tris: int = 0, split: int = 0,
               device: int = 0):
        _keep, args = _scene_arrays(geoms, geom_ids, tris, tri_ids, tri_albedo, tri_tex, textures)
        h = C.c_void_p()
        bp = SvgfSceneBuildParams(int(max_leaf_tris), int(split))
        _call(load_library(), "svgf_scene_create", int(device), *args, C.byref(bp), C.byref(h))
        return cls(h, device)

    def _call(self, symbol, *args):
        _call(self.lib, symbol, self.h, *args)

    def info(self) -> dict:
        i = SvgfSceneInfo()
        self._call("svgf_scene_info", C.byref(i))
        return {k: int(getattr(i, k)) for k, _ in SvgfSceneInfo._fields_}

    def draw(self, out_rgb, out_gbuffer, width: int, height: int, camera, light, frame: int, seed: int = 1, noise: float = 0.6,
             fireflies: float = 0.02, pixel_length=None, stream=None):
        """svgf_scene_draw, or svgf_scene_draw_planar when `out_gbuffer` is a SvgfPlanarGBuffer.  Asynchronous on `stream` (a torch
        stream, a raw handle or None = the default stream); never waits."""
        cam, sp = _view(camera, width, height, frame, seed, noise, fireflies, pixel_length, camera_fovy=True)
        planar, texels, planes = _draw_target(out_gbuffer)
        fn = self.lib.svgf_scene_draw_planar if planar else self.lib.svgf_scene_draw
        _check(fn(self.h, _ptr(out_rgb), planes if planar else texels, int(width), int(height), C.byref(cam), C.byref(sp), _v3(light),
                  _stream(stream)), "svgf_scene_draw")      # one name for both in the message

    draw_planar = draw

    def draw_shadowed(self, out_rgb, out_gbuffer, width: int, height: int, camera, light, frame: int, seed: int = 1, noise: float = 0.6,
                      fireflies: float = 0.02, pixel_length=None, stream=None):
        """svgf_scene_draw_shadowed (row f16): `light` is a SvgfSceneLight (SvgfSceneLight.make(centre, edge_u, edge_v, samples));
        `out_gbuffer` AoS texels or a SvgfPlanarGBuffer.  One launch on `stream`; never waits."""
        cam, sp = _view(camera, width, height, frame, seed, noise, fireflies, pixel_length, camera_fovy=True)
        self._call("svgf_scene_draw_shadowed", _ptr(out_rgb), *_draw_target(out_gbuffer)[1:], int(width), int(height), C.byref(cam), C.byref(sp),
                   C.byref(light), _stream(stream))

    def _companion_draw(self, name, out, out_gbuffer, width, height, camera, light, frame, params, synth, stream, table=None, guide=None,
                        lobe=None, shine=None):
        """One draw of libsvgf_<name>.so, every companion's the same way.  `out` is (out_rgb,) or, for the split form, (out_direct,
        out_indirect, out_rgb); `params` the values of the library's parameter block, `synth` (seed, noise, fireflies, pixel_length);
        the libraries that take them read `table` (a GlossTable or None), `guide` (max_chain, id_offset, out_chain), `lobe` (a RoughTable
        or None, guide_alpha) and `shine` (enable, clamp).  `out_gbuffer` is AoS texels or a SvgfPlanarGBuffer."""
        parts = _DRAW_PARTS["trace" if name == "split" else name]
        symbol = ("svgf_trace_draw" if name == "split" else f"svgf_{name}_draw") + "_split" * (len(out) == 3)
        cam, sp = _view(camera, width, height, frame, *synth, camera_fovy=True)
        args = [self.h] + ([table.h if table is not None else None] if parts.get("table") else []) + [_ptr(o) for o in out]
        args += [*_draw_target(out_gbuffer)[1:], int(width), int(height), C.byref(cam), C.byref(sp), C.byref(light),
                 C.byref(_filled(parts["params"], params))]
        if parts.get("virtual"):
            args += [C.byref(_filled(SvgfVirtualParams, guide[:2])), _ptr(guide[2])]
        args.append(_stream(stream))
        if parts.get("rough"):
            args += [lobe[0].h if lobe[0] is not None else None, C.byref(_filled(SvgfRoughParams, lobe[1:]))]
        if parts.get("highlight"):
            args.append(C.byref(_filled(SvgfHighlightParams, shine)))
        _call(_load_companion(name), symbol, *args)

    def draw_traced(self, out_rgb, out_gbuffer, width: int, height: int, camera, light, frame: int, bounce_samples: int = 1,
                    ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1, noise: float = 0.6, fireflies: float = 0.02,
                    pixel_length=None, stream=None):
        """svgf_trace_draw of libsvgf_trace.so (row f17): draw_shadowed's frame plus one diffuse bounce gathered over
        `bounce_samples` directions.  One launch on `stream`; never waits."""
        self._companion_draw("trace", (out_rgb,), out_gbuffer, width, height, camera, light, frame,
                             (bounce_samples, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream)

    def draw_traced_split(self, out_direct, out_indirect, out_gbuffer, width: int, height: int, camera, light, frame: int,
                          bounce_samples: int = 1, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1, noise: float = 0.6,
                          fireflies: float = 0.02, pixel_length=None, out_rgb=None, stream=None):
        """svgf_trace_draw_split of libsvgf_split.so (row f18): draw_traced's rays, with the direct and the indirect term written
        apart and without the albedo; `out_rgb` (optional) receives draw_traced's colour.  One launch on `stream`; never waits."""
        self._companion_draw("split", (out_direct, out_indirect, out_rgb), out_gbuffer, width, height, camera, light, frame,
                             (bounce_samples, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream)

    def draw_path(self, out_rgb, out_gbuffer, width: int, height: int, camera, light, frame: int, paths: int = 1, max_depth: int = 4,
                  rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1, noise: float = 0.6,
                  fireflies: float = 0.02, pixel_length=None, stream=None):
        """svgf_path_draw of libsvgf_path.so (row f19): draw_traced's frame with `paths` paths of up to `max_depth` diffuse bounces per
        pixel in the one bounce's place, Russian roulette from bounce `rr_depth` on (0: none).  One launch on `stream`; never waits."""
        self._companion_draw("path", (out_rgb,), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream)

    def draw_path_split(self, out_direct, out_indirect, out_gbuffer, width: int, height: int, camera, light, frame: int, paths: int = 1,
                        max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1,
                        noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, out_rgb=None, stream=None):
        """svgf_path_draw_split of libsvgf_path.so (row f19): draw_path's rays, with the direct and the indirect term written apart and
        without the albedo; `out_rgb` (optional) receives draw_path's colour.  One launch on `stream`; never waits."""
        self._companion_draw("path", (out_direct, out_indirect, out_rgb), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream)

    def draw_gloss(self, out_rgb, out_gbuffer, width: int, height: int, camera, light, frame: int, table=None, paths: int = 1,
                   max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1, noise: float = 0.6,
                   fireflies: float = 0.02, pixel_length=None, stream=None):
        """svgf_gloss_draw of libsvgf_gloss.so (row f20): draw_path's frame with the mirror and glass surfaces of `table` (a GlossTable,
        or None: every surface diffuse, draw_path's frame on bits) along the paths.  One launch on `stream`; never waits."""
        self._companion_draw("gloss", (out_rgb,), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream, table)

    def draw_gloss_split(self, out_direct, out_indirect, out_gbuffer, width: int, height: int, camera, light, frame: int, table=None,
                         paths: int = 1, max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1,
                         noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, out_rgb=None, stream=None):
        """svgf_gloss_draw_split of libsvgf_gloss.so (row f20): draw_gloss's rays, with the direct and the indirect term written apart
        and without the albedo; `out_rgb` (optional) receives draw_gloss's colour.  One launch on `stream`; never waits."""
        self._companion_draw("gloss", (out_direct, out_indirect, out_rgb), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream, table)

    def draw_virtual(self, out_rgb, out_gbuffer, width: int, height: int, camera, light, frame: int, table=None, paths: int = 1,
                     max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1, noise: float = 0.6,
                     fireflies: float = 0.02, pixel_length=None, stream=None, max_chain: int = 4, id_offset: int = 0, out_chain=None):
        """svgf_virtual_draw of libsvgf_virtual.so (row f21): draw_gloss's frame, on bits, with a G-buffer whose normal, position and
        geomId describe what a full mirror or glass shows (a guide chain of at most `max_chain` rays; `id_offset` is added to a virtual
        hit's id).  `out_chain` (optional) receives one int32 per pixel.  One launch on `stream`; never waits."""
        self._companion_draw("virtual", (out_rgb,), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream, table,
                             (max_chain, id_offset, out_chain))

    def draw_virtual_split(self, out_direct, out_indirect, out_gbuffer, width: int, height: int, camera, light, frame: int, table=None,
                           paths: int = 1, max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1,
                           noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, out_rgb=None, stream=None, max_chain: int = 4,
                           id_offset: int = 0, out_chain=None):
        """svgf_virtual_draw_split of libsvgf_virtual.so (row f21): draw_gloss_split's D, I and colour, on bits, with draw_virtual's
        G-buffer.  One launch on `stream`; never waits."""
        self._companion_draw("virtual", (out_direct, out_indirect, out_rgb), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream, table,
                             (max_chain, id_offset, out_chain))

    def draw_rough(self, out_rgb, out_gbuffer, width: int, height: int, camera, light, frame: int, table=None, paths: int = 1,
                   max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1, noise: float = 0.6,
                   fireflies: float = 0.02, pixel_length=None, stream=None, max_chain: int = 4, id_offset: int = 0, out_chain=None, rough=None,
                   guide_alpha: float = 0.0):
        """svgf_rough_draw of libsvgf_rough.so (row f22): draw_virtual with a GGX lobe on the mirror vertices of the objects the
        RoughTable `rough` gives a roughness; the guide follows a full mirror no rougher than `guide_alpha`.  With rough=None it is
        draw_virtual's frame on bits.  One launch on `stream`; never waits."""
        self._companion_draw("rough", (out_rgb,), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream, table,
                             (max_chain, id_offset, out_chain), (rough, guide_alpha))

    def draw_rough_split(self, out_direct, out_indirect, out_gbuffer, width: int, height: int, camera, light, frame: int, table=None,
                         paths: int = 1, max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1,
                         noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, out_rgb=None, stream=None, max_chain: int = 4,
                         id_offset: int = 0, out_chain=None, rough=None, guide_alpha: float = 0.0):
        """svgf_rough_draw_split of libsvgf_rough.so (row f22): draw_virtual_split with draw_rough's lobe and guide.  One launch on
        `stream`; never waits."""
        self._companion_draw("rough", (out_direct, out_indirect, out_rgb), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream, table,
                             (max_chain, id_offset, out_chain), (rough, guide_alpha))

    def draw_highlight(self, out_rgb, out_gbuffer, width: int, height: int, camera, light, frame: int, table=None, paths: int = 1,
                       max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1, seed: int = 1, noise: float = 0.6,
                       fireflies: float = 0.02, pixel_length=None, stream=None, max_chain: int = 4, id_offset: int = 0, out_chain=None, rough=None,
                       guide_alpha: float = 0.0, enable: int = 1, clamp: float = 0.0):
        """svgf_highlight_draw of libsvgf_highlight.so (row f23): draw_rough with the analytic light's GGX term at the rough vertices
        (`enable` 1), its scalar factor clamped to `clamp` where that is above 0.  With enable=0 it is draw_rough's frame on bits.  One
        launch on `stream`; never waits."""
        self._companion_draw("highlight", (out_rgb,), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream, table,
                             (max_chain, id_offset, out_chain), (rough, guide_alpha), (enable, clamp))

    def draw_highlight_split(self, out_direct, out_indirect, out_gbuffer, width: int, height: int, camera, light, frame: int, table=None,
                             paths: int = 1, max_depth: int = 4, rr_depth: int = 2, ambient: float = 0.15, shadow_secondary: int = 1,
                             seed: int = 1, noise: float = 0.6, fireflies: float = 0.02, pixel_length=None, out_rgb=None, stream=None,
                             max_chain: int = 4, id_offset: int = 0, out_chain=None, rough=None, guide_alpha: float = 0.0, enable: int = 1,
                             clamp: float = 0.0):
        """svgf_highlight_draw_split of libsvgf_highlight.so (row f23): draw_rough_split with draw_highlight's term; at the first hit
        it is part of the direct image.  One launch on `stream`; never waits."""
        self._companion_draw("highlight", (out_direct, out_indirect, out_rgb), out_gbuffer, width, height, camera, light, frame,
                             (paths, max_depth, rr_depth, ambient, shadow_secondary), (seed, noise, fireflies, pixel_length), stream, table,
                             (max_chain, id_offset, out_chain), (rough, guide_alpha), (enable, clamp))

    def adopt_tree(self, nodes=None, order=None, n_nodes: int = 0, n_leaves: int = 0, depth_bound: int = 0):
        """svgf_scene_adopt_tree (row f24; host only): from now on every draw walks the DEVICE arrays `nodes` / `order` (torch tensors
        or raw pointers) in place of the scene's own tree; nodes=None detaches.  SceneTree.attach() does this with a tree it built."""
        self._call("svgf_scene_adopt_tree", _ptr(nodes), _ptr(order), int(n_nodes), int(n_leaves), int(depth_bound))

    def view(self) -> dict:
        """svgf_scene_view (host only): the device index, the counts and the device pointers the draws read, as integers (0 = NULL)."""
        v = SvgfSceneView()
        self._call("svgf_scene_view", C.byref(v))
        return {k: int(getattr(v, k) or 0) for k, _ in SvgfSceneView._fields_}

    def enable_pose(self, n_objects: int):
        """svgf_scene_enable_pose: allocates the animation side (allocates and synchronises; not under capture)."""
        self._call("svgf_scene_enable_pose", int(n_objects))
        self.n_objects = int(n_objects)

    def pose(self, table, motion_out=None, stream=None):
        """svgf_scene_pose: `table` is DEVICE memory of n_objects SCENE_POSE_DTYPE records (a torch tensor of 24 * n_objects float32
        or a raw pointer), read when the kernels run; `motion_out` device memory of 12 * n_objects float32 or None.  Asynchronous on
        `stream`; never waits."""
        self._call("svgf_scene_pose", _ptr(table), int(getattr(self, "n_objects", 0)), _ptr(motion_out), _stream(stream))

    def read(self, which: int) -> np.ndarray:
        """svgf_scene_read (blocking): 0 float32[n_tris, 3, 8], 1 / 2 BVH_NODE_DTYPE, 3 scene.SCENE_GEOM_DTYPE, 4 int32, 5 SCENE_POSE_DTYPE."""
        from . import scene as _scene
        i = self.info()
        n, dt = {0: (i["n_tris"] * 24, np.float32), 1: (i["n_tris"], BVH_NODE_DTYPE), 2: (i["n_nodes"], BVH_NODE_DTYPE),
                 3: (i["n_geoms"], _scene.SCENE_GEOM_DTYPE), 4: (i["n_tris"], np.int32),
                 5: (getattr(self, "n_objects", 0), SCENE_POSE_DTYPE)}[int(which)]
        out = np.zeros(n, dt)
        self._call("svgf_scene_read", int(which), out.ctypes.data if n else None, out.nbytes)
        return out.reshape(-1, 3, 8) if int(which) == 0 else out

    def free(self):
        if self.h:
            self.lib.svgf_scene_destroy(self.h)
            self.h = None


class SceneTree:
    """A linear BVH over a resident scene's triangles as drawn, built on the device by libsvgf_lbvh.so (row f24): create once (one
    allocation; not under capture), build(stream) per frame behind the pose - info()["launches"] kernel launches and nothing else, legal
    under capture - attach() once, detach() before free().  Usable as a context manager."""

    def __init__(self, handle, scene):
        self.lib, self.h, self.scene = load_lbvh_library(), handle, scene

    @classmethod
    def create(cls, scene, leaf_tris: int = 0):
        h, p = C.c_void_p(), SvgfLbvhParams(int(leaf_tris))
        _call(load_lbvh_library(), "svgf_lbvh_create", scene.h, C.byref(p), C.byref(h))
        return cls(h, scene)

    def _call(self, symbol, *args):
        _call(self.lib, symbol, self.h, *args)

    def build(self, stream=None):
        """svgf_lbvh_build: asynchronous on `stream`; never waits."""
        self._call("svgf_lbvh_build", _stream(stream))

    def attach(self):
        self._call("svgf_lbvh_attach", self.scene.h)

    def detach(self):
        self.scene.adopt_tree(None)

    def info(self) -> dict:
        i = SvgfLbvhInfo()
        self._call("svgf_lbvh_info", C.byref(i))
        return {k: int(getattr(i, k)) for k, _ in SvgfLbvhInfo._fields_}

    def read(self, which: int) -> np.ndarray:
        """svgf_lbvh_read (blocking): 0 nodes BVH_NODE_DTYPE[n_nodes], 1 order int32[n_tris], 2 the sorted keys uint64[n_tris]."""
        i = self.info()
        n, dt = {0: (i["n_nodes"], BVH_NODE_DTYPE), 1: (i["n_tris"], np.int32), 2: (i["n_tris"], np.uint64)}[int(which)]
        out = np.zeros(n, dt)
        self._call("svgf_lbvh_read", int(which), out.ctypes.data, out.nbytes)
        return out

    def free(self):
        if self.h:
            self.lib.svgf_lbvh_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


ResidentScene = Scene
