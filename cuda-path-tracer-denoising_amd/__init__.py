"""MI355X-native SVGF denoiser behind the reference's denoise.h entry points.

Directory layout:
  csrc/                HIP kernels (gfx950) + the C ABI of include/svgf.h  -> libsvgf_hip.so (built in-tree)
  binding.py           ctypes binding + `Denoiser`, the host-side mirror of denoiseInit/denoise/denoiseFree
  farm.py              sequence sharding + timing reduction for the 1/2/4/8-GPU runs (no collectives on the data path)
  synth.py             seeded synthetic 1-spp colour + G-buffer frames (test / bench inputs)
  sah.py               ctypes binding of libsvgf_sah.so (row f25): `SahTree`, the device SAH build of a resident scene's tree
  deform.py            ctypes binding of libsvgf_deform.so (row f26): `DeformRig`, skinned triangles; scene_refit / drawn_arrays of the product
  restir.py            ctypes binding of libsvgf_restir.so (row f27): `LightTable`, `Restir`, many-light direct lighting by reservoir resampling
  restir_gi.py         ctypes binding of libsvgf_restir_gi.so (row f28): `RestirGI`, the one-bounce indirect term by reservoir resampling
  build.py             hipcc / gcc recipes used by __graft_entry__.build()
The directory name contains '-', so it is loaded through `__graft_entry__.load_package()` under the module
name `cuda_path_tracer_denoising_amd`.
"""
from . import binding, build, deform, farm, restir, restir_gi, sah, scene, synth  # noqa: F401
from .binding import Denoiser, SvgfCamera, SvgfParams, SvgfError, load_library, reference_defaults  # noqa: F401
from .binding import SvgfGuide, SvgfUpsampleParams, upsample  # noqa: F401
from .binding import SvgfExposureParams, SvgfTonemapParams, exposure_state, exposure_reset, exposure_meter, display_tonemap, srgb_table  # noqa: F401
from .binding import SvgfQualityParams, SvgfQualityResult, quality_state, quality_windows, quality_meter, quality_read  # noqa: F401
from .binding import Scene, SvgfSceneBuildParams, SvgfSceneInfo, bvh_build_host  # noqa: F401
from .binding import ResidentScene, SCENE_POSE_DTYPE, pose_rigid, pose_identity, bvh_refit_plan_host  # noqa: F401
from .binding import SvgfSceneLight  # noqa: F401
from .binding import SvgfSceneView, SvgfTraceParams, load_trace_library  # noqa: F401
from .binding import load_split_library, trace_compose  # noqa: F401  (Scene.draw_traced_split is its other half)
from .binding import SvgfPathParams, load_path_library  # noqa: F401  (Scene.draw_path, Scene.draw_path_split)
from .binding import GlossTable, SvgfSurface, load_gloss_library  # noqa: F401  (Scene.draw_gloss, Scene.draw_gloss_split)
from .binding import SvgfVirtualParams, load_virtual_library  # noqa: F401  (Scene.draw_virtual, Scene.draw_virtual_split)
from .binding import RoughTable, SvgfRoughParams, load_rough_library  # noqa: F401  (Scene.draw_rough, Scene.draw_rough_split)
from .binding import SvgfHighlightParams, load_highlight_library  # noqa: F401  (Scene.draw_highlight, Scene.draw_highlight_split)
from .binding import SceneTree, SvgfLbvhParams, SvgfLbvhInfo, load_lbvh_library, lbvh_build_host  # noqa: F401  (row f24, Scene.adopt_tree)
from .sah import SahTree, SvgfSahParams, SvgfSahInfo, SAH_EXPORTS, load_sah_library  # noqa: F401  (row f25)
from .deform import DeformRig, SvgfDeformInfo, DEFORM_EXPORTS, SCENE_WRITE_EXPORTS, load_deform_library, scene_refit, drawn_arrays  # noqa: F401  (row f26)
from .restir import LightTable, Restir, SvgfLight, SvgfRestirParams, SvgfRestirInfo, RESTIR_EXPORTS, load_restir_library  # noqa: F401  (row f27)
from .restir_gi import RestirGI, SvgfRestirGIParams, SvgfRestirGIInfo, RESTIR_GI_EXPORTS, RESERVOIR_GI_DTYPE, gi_params, load_restir_gi_library  # noqa: F401  (row f28)
from .binding import STATE_PREV_NORMAL, STATE_PREV_POSITION, STATE_PREV_GEOM_ID, STATE_OUTPUT_HISTORY  # noqa: F401
