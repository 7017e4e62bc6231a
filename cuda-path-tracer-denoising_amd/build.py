"""Build recipe of the product library (no cmake, no JIT cache): everything lands in-tree so it travels to the GPU box.
The checkers (CPU restatement, the reference's own denoise.cu) have their own recipe outside this package."""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
LIB = os.path.join(_HERE, "libsvgf_hip.so")
# The experiments build (-DSVGF_BUILD_EXPERIMENTS): the product's sources + the parked kernel variants and the tuning table
# (svgf_exp_set).  Test / tools infrastructure: nothing on the product path loads it (binding.load_library(experiments=True) does).
LIB_EXP = os.path.join(_HERE, "libsvgf_hip_exp.so")

HIP_SOURCES = ["svgf_api.hip", "svgf_frame.hip", "svgf_pipeline.hip", "svgf_profiler.hip", "svgf_kernels.hip", "svgf_atrous_geometry.hip", "svgf_atrous_strip.hip", "svgf_atrous_lane.hip", "svgf_atrous_prepare_fused.hip", "svgf_atrous_lattice.hip", "svgf_synth.hip", "svgf_scene.hip", "svgf_display.hip", "svgf_upsample.hip", "svgf_transfer.hip", "svgf_quality.hip", "svgf_scene_bvh.hip"]
# plain C++ (no HIP in them; compiled as C++, for the host only): the resident scene's BVH builder
CXX_SOURCES = ["svgf_bvh_build.cpp"]
CXX_FLAGS = ["-x", "c++", "-O3", "-std=c++17", "-fPIC", "-Wall", "-ffp-contract=off"]
# The companion library of row f17 (include/svgf_trace.h: the path-traced draw): renderer-side code, built from the same tree and
# linked against the product library, which stays what it was (tests/test_abi.py caps its size).
LIB_TRACE = os.path.join(_HERE, "libsvgf_trace.so")
TRACE_SOURCES = ["svgf_scene_trace.hip"]
# The companion library of row f18 (include/svgf_split.h: the split draw and the recomposition): a second one, so that libsvgf_trace.so
# stays the two functions it was; its draw compiles the same kernel text (csrc/svgf_scene_trace.inc.h).
LIB_SPLIT = os.path.join(_HERE, "libsvgf_split.so")
SPLIT_SOURCES = ["svgf_scene_split.hip", "svgf_trace_compose.hip"]
# The companion library of row f19 (include/svgf_path.h: paths of several bounces with roulette, plain and split): a third one, so that
# the other two stay the code objects they were; its kernel compiles the same shared texts (csrc/svgf_scene_trace.inc.h and below).
LIB_PATH = os.path.join(_HERE, "libsvgf_path.so")
PATH_SOURCES = ["svgf_scene_path.hip"]
# The companion library of row f20 (include/svgf_gloss.h: the paths with a mirror and a glass lobe per object): a fourth one, so that
# the other three stay the code objects they were; its kernel compiles the same shared texts unchanged.
LIB_GLOSS = os.path.join(_HERE, "libsvgf_gloss.so")
GLOSS_SOURCES = ["svgf_scene_gloss.hip"]
# The companion library of row f21 (include/svgf_virtual.h: the glossy draws with a virtual-hit G-buffer): a fifth one; its kernel is
# csrc/svgf_scene_gloss.inc.h's, the text libsvgf_gloss.so compiles, and that library's code object stays what it was.
LIB_VIRTUAL = os.path.join(_HERE, "libsvgf_virtual.so")
VIRTUAL_SOURCES = ["svgf_scene_virtual.hip"]
# The companion library of row f22 (include/svgf_rough.h: the virtual-hit draws with a GGX lobe on rough mirrors): a sixth one; its
# kernel is csrc/svgf_scene_gloss.inc.h's too, and the gloss and the virtual library's code objects stay what they were.
LIB_ROUGH = os.path.join(_HERE, "libsvgf_rough.so")
ROUGH_SOURCES = ["svgf_scene_rough.hip"]
# The companion library of row f23 (include/svgf_highlight.h: the rough draws with the light's GGX term at rough vertices): a seventh
# one; its kernel is csrc/svgf_scene_gloss.inc.h's too, and the gloss, virtual and rough libraries' code objects stay what they were.
LIB_HIGHLIGHT = os.path.join(_HERE, "libsvgf_highlight.so")
HIGHLIGHT_SOURCES = ["svgf_scene_highlight.hip"]
HIP_SOURCES_EXPERIMENTS = ["svgf_experiments.hip", "svgf_atrous_lane_reuse.hip", "svgf_atrous_fused.hip"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function"]
# Per-file flags.  svgf_atrous_fused.hip: SimplifyCFG's common-code sinking merges the last store of the "bilinear history" branch
# with the last store of the "fallback consistency data" branch of the temporal stage into ONE store through a phi of two
# pointers, which keeps those request registers in scratch memory (every load followed by s_waitcnt vmcnt(0) + scratch_store).
HIPCC_FILE_FLAGS = {"svgf_atrous_fused.hip": ["-mllvm", "-simplifycfg-sink-common=false"]}


def _newer(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _run(cmd: list[str], cwd: str | None = None):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed: " + " ".join(cmd) + "\n" + r.stdout)
    return r.stdout


def hipcc_path() -> str:
    p = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(p):
        raise RuntimeError("hipcc not found")
    return p


def build_hip(force: bool = False, experiments: bool = False) -> str:
    """Compile the HIP kernels + C ABI for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_hip.so (the product), or, with
    experiments=True, into libsvgf_hip_exp.so (-DSVGF_BUILD_EXPERIMENTS: parked kernel variants 5 / 6, cross-level term reuse, the
    tuning table behind svgf_exp_set; what tools/experiments/ and the tests marked `experiments` load)."""
    LIB = LIB_EXP if experiments else globals()["LIB"]
    srcs = [os.path.join(CSRC, s) for s in HIP_SOURCES + (HIP_SOURCES_EXPERIMENTS if experiments else []) + CXX_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + [os.path.join(ROOT, "include", "svgf.h")]
    if not force and _newer(LIB, deps):
        return LIB
    tmp = LIB + f".tmp{os.getpid()}"
    extra = os.environ.get("SVGF_EXTRA_HIPCC_FLAGS", "").split() if experiments else []      # -D switches of tools/experiments/ (experiments build only)
    if experiments:
        extra = ["-DSVGF_BUILD_EXPERIMENTS"] + extra
    # one hipcc -c per translation unit, in parallel (the a-trous kernels are template-heavy: ~70 s serial, ~30 s so),
    # objects in a scratch directory, then one link
    import concurrent.futures
    import tempfile
    cflags = [f for f in HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory(prefix="svgf_build_") as scratch:
        objs = [os.path.join(scratch, os.path.basename(x) + ".o") for x in srcs]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 1)) as pool:
            list(pool.map(lambda so: _run([hipcc_path()] + (CXX_FLAGS if os.path.basename(so[0]) in CXX_SOURCES else
                                                            cflags + HIPCC_FILE_FLAGS.get(os.path.basename(so[0]), []) + extra) + ["-c", so[0], "-o", so[1]]),
                          zip(srcs, objs)))
        # the product library is linked stripped (-Wl,-s: host side, link line only): .symtab / .strtab go, the dynamic symbols and
        # the device code objects (.dynsym, .hip_fatbin) stay; DESIGN.md 5.4g has the sizes with and without
        _run([hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC"] + ([] if experiments else ["-Wl,-s"]) + objs + ["-o", tmp])
    os.replace(tmp, LIB)              # atomic: concurrent ranks never see a half-written library
    return LIB


def build_trace(force: bool = False) -> str:
    """Compile csrc/svgf_scene_trace.hip for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_trace.so, linked against the product
    library beside it (the examples' rpath scheme: the build directory, then $ORIGIN, so the pair can be moved together)."""
    build_hip()
    srcs = [os.path.join(CSRC, s) for s in TRACE_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
        [os.path.join(ROOT, "include", "svgf.h"), os.path.join(ROOT, "include", "svgf_trace.h"), LIB]
    if not force and _newer(LIB_TRACE, deps):
        return LIB_TRACE
    tmp = LIB_TRACE + f".tmp{os.getpid()}"
    _run([hipcc_path()] + HIPCC_FLAGS + srcs + ["-L", _HERE, "-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN", "-Wl,-s", "-o", tmp])
    os.replace(tmp, LIB_TRACE)
    return LIB_TRACE


def build_split(force: bool = False) -> str:
    """Compile csrc/svgf_scene_split.hip and csrc/svgf_trace_compose.hip for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_split.so,
    linked against the product library beside it, by build_trace()'s scheme."""
    build_hip()
    srcs = [os.path.join(CSRC, s) for s in SPLIT_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
        [os.path.join(ROOT, "include", h) for h in ("svgf.h", "svgf_trace.h", "svgf_split.h")] + [LIB]
    if not force and _newer(LIB_SPLIT, deps):
        return LIB_SPLIT
    tmp = LIB_SPLIT + f".tmp{os.getpid()}"
    _run([hipcc_path()] + HIPCC_FLAGS + srcs + ["-L", _HERE, "-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN", "-Wl,-s", "-o", tmp])
    os.replace(tmp, LIB_SPLIT)
    return LIB_SPLIT


def build_path(force: bool = False) -> str:
    """Compile csrc/svgf_scene_path.hip for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_path.so, linked against the product
    library beside it (and against neither other companion), by build_trace()'s scheme."""
    build_hip()
    srcs = [os.path.join(CSRC, s) for s in PATH_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
        [os.path.join(ROOT, "include", h) for h in ("svgf.h", "svgf_trace.h", "svgf_path.h")] + [LIB]
    if not force and _newer(LIB_PATH, deps):
        return LIB_PATH
    tmp = LIB_PATH + f".tmp{os.getpid()}"
    _run([hipcc_path()] + HIPCC_FLAGS + srcs + ["-L", _HERE, "-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN", "-Wl,-s", "-o", tmp])
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def build_gloss(force: bool = False) -> str:
    """Compile csrc/svgf_scene_gloss.hip for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_gloss.so, linked against the product
    library beside it (and against no other companion), by build_trace()'s scheme."""
    build_hip()
    srcs = [os.path.join(CSRC, s) for s in GLOSS_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
        [os.path.join(ROOT, "include", h) for h in ("svgf.h", "svgf_trace.h", "svgf_path.h", "svgf_gloss.h")] + [LIB]
    if not force and _newer(LIB_GLOSS, deps):
        return LIB_GLOSS
    tmp = LIB_GLOSS + f".tmp{os.getpid()}"
    _run([hipcc_path()] + HIPCC_FLAGS + srcs + ["-L", _HERE, "-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN", "-Wl,-s", "-o", tmp])
    os.replace(tmp, LIB_GLOSS)
    return LIB_GLOSS


def build_virtual(force: bool = False) -> str:
    """Compile csrc/svgf_scene_virtual.hip for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_virtual.so, linked against the product
    library beside it (and against no other companion: a svgf_gloss_table is read through csrc/svgf_gloss_table.h), by build_trace()'s
    scheme."""
    build_hip()
    srcs = [os.path.join(CSRC, s) for s in VIRTUAL_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
        [os.path.join(ROOT, "include", h) for h in ("svgf.h", "svgf_trace.h", "svgf_path.h", "svgf_gloss.h", "svgf_virtual.h")] + [LIB]
    if not force and _newer(LIB_VIRTUAL, deps):
        return LIB_VIRTUAL
    tmp = LIB_VIRTUAL + f".tmp{os.getpid()}"
    _run([hipcc_path()] + HIPCC_FLAGS + srcs + ["-L", _HERE, "-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN", "-Wl,-s", "-o", tmp])
    os.replace(tmp, LIB_VIRTUAL)
    return LIB_VIRTUAL


def build_rough(force: bool = False) -> str:
    """Compile csrc/svgf_scene_rough.hip for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_rough.so, linked against the product
    library beside it (and against no other companion), by build_trace()'s scheme."""
    build_hip()
    srcs = [os.path.join(CSRC, s) for s in ROUGH_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
        [os.path.join(ROOT, "include", h) for h in ("svgf.h", "svgf_trace.h", "svgf_path.h", "svgf_gloss.h", "svgf_virtual.h", "svgf_rough.h")] + [LIB]
    if not force and _newer(LIB_ROUGH, deps):
        return LIB_ROUGH
    tmp = LIB_ROUGH + f".tmp{os.getpid()}"
    _run([hipcc_path()] + HIPCC_FLAGS + srcs + ["-L", _HERE, "-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN", "-Wl,-s", "-o", tmp])
    os.replace(tmp, LIB_ROUGH)
    return LIB_ROUGH


def build_highlight(force: bool = False) -> str:
    """Compile csrc/svgf_scene_highlight.hip for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_highlight.so, linked against the
    product library beside it (and against no other companion: the two tables are read through csrc/svgf_gloss_table.h and
    csrc/svgf_rough_table.h), by build_trace()'s scheme."""
    build_hip()
    srcs = [os.path.join(CSRC, s) for s in HIGHLIGHT_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
        [os.path.join(ROOT, "include", h) for h in ("svgf.h", "svgf_trace.h", "svgf_path.h", "svgf_gloss.h", "svgf_virtual.h", "svgf_rough.h",
                                                    "svgf_highlight.h")] + [LIB]
    if not force and _newer(LIB_HIGHLIGHT, deps):
        return LIB_HIGHLIGHT
    tmp = LIB_HIGHLIGHT + f".tmp{os.getpid()}"
    _run([hipcc_path()] + HIPCC_FLAGS + srcs + ["-L", _HERE, "-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN", "-Wl,-s", "-o", tmp])
    os.replace(tmp, LIB_HIGHLIGHT)
    return LIB_HIGHLIGHT


def build_all(force: bool = False) -> list[str]:
    """The product library and the seven companion libraries, in the order they were added."""
    return [build_hip(force), build_trace(force), build_split(force), build_path(force), build_gloss(force), build_virtual(force), build_rough(force),
            build_highlight(force)]


def build_examples(force: bool = False) -> str:
    """examples/farm.cpp (N contexts on N GPUs from one C++ process), examples/pipeline.cpp (a renderer's frame loop on the frame
    pipeline), examples/cadence.cpp (a fixed-rate loop + the effective shader clock), examples/upsample.cpp (denoise at a reduced
    size, svgf_upsample to the full size), examples/dynres.cpp (the reduced size changes every few frames,
    svgf_transfer_history carries the sequence along), examples/hdr_display.cpp (an emitter far above 1: svgf_exposure_meter on
    the denoised image, svgf_display_tonemap beside the plain pack) and examples/quality.cpp (svgf_quality_meter: PSNR / SSIM of the
    noisy and the denoised frame against the clean one, and of consecutive outputs) and examples/resident_scene.cpp (svgf_scene_create
    once, then svgf_scene_draw + svgf_denoise per frame) and examples/animated_scene.cpp (svgf_scene_pose with a motion table ahead of
    each draw) and examples/shadowed_scene.cpp (svgf_scene_draw_shadowed: one shadow ray per pixel, denoised, against 64), through the C ABI -> examples/farm, examples/pipeline, examples/cadence, examples/upsample, examples/dynres,
    examples/hdr_display, examples/quality, examples/resident_scene, examples/animated_scene, examples/shadowed_scene, linked against the product library
    in-tree; and examples/traced_scene.cpp (svgf_trace_draw: one bounce sample and one shadow ray per pixel, denoised three ways,
    against a converged frame) and examples/split_scene.cpp (svgf_trace_draw_split, a context per term, svgf_trace_compose: SVGF's
    own pipeline beside the one-image one), linked against both companion libraries; and examples/path_scene.cpp (svgf_path_draw and
    svgf_path_draw_split at depth 1 and 4, each denoised as one image and as two), linked against the path and the split library; and
    examples/gloss_scene.cpp (svgf_gloss_draw_split on a room with a mirror sphere and a glass cube, the two-context pipeline with and
    without the history clamp, scored inside and outside the mirror), linked against the gloss and the split library; and
    examples/virtual_scene.cpp (the same room through the same pipeline with the first-hit and with the virtual-hit G-buffer of
    svgf_virtual_draw_split), linked against the virtual, the gloss and the split library; and examples/rough_scene.cpp (that room with
    a rough floor through the same pipeline, svgf_rough_draw_split with guide_alpha 0 and 1, with and without the firefly filter and the
    history clamp), linked against the rough, the gloss and the split library; and examples/highlight_scene.cpp (that room and floor under
    svgf_highlight_draw_split with the highlight off, on and clamped, both terms with and without the firefly filter and the history clamp),
    linked against the highlight, the rough, the gloss and the split library."""
    build_trace()
    build_split()
    build_path()
    build_gloss()
    build_virtual()
    build_rough()
    build_highlight()
    out = ""
    for name in ("pipeline", "farm", "cadence", "upsample", "dynres", "hdr_display", "quality", "resident_scene", "animated_scene", "shadowed_scene", "traced_scene", "split_scene", "path_scene", "gloss_scene", "virtual_scene", "rough_scene", "highlight_scene"):
        src = os.path.join(ROOT, "examples", name + ".cpp")
        out = os.path.join(ROOT, "examples", name)
        traced, split, path = name in ("traced_scene", "split_scene"), name in ("split_scene", "path_scene", "gloss_scene", "virtual_scene", "rough_scene", "highlight_scene"), name == "path_scene"
        gloss, virt, rough = name in ("gloss_scene", "virtual_scene", "rough_scene", "highlight_scene"), name == "virtual_scene", name in ("rough_scene", "highlight_scene")
        shine = name == "highlight_scene"
        if not force and _newer(out, [src, os.path.join(ROOT, "include", "svgf.h"), LIB] + ([os.path.join(ROOT, "include", "svgf_trace.h"), LIB_TRACE] if traced else []) +
                                ([os.path.join(ROOT, "include", "svgf_split.h"), LIB_SPLIT] if split else []) +
                                ([os.path.join(ROOT, "include", "svgf_path.h"), LIB_PATH] if path else []) +
                                ([os.path.join(ROOT, "include", "svgf_gloss.h"), os.path.join(ROOT, "include", "svgf_path.h"), LIB_GLOSS] if gloss else []) +
                                ([os.path.join(ROOT, "include", "svgf_virtual.h"), LIB_VIRTUAL] if virt else []) +
                                ([os.path.join(ROOT, "include", "svgf_rough.h"), os.path.join(ROOT, "include", "svgf_virtual.h"), LIB_ROUGH] if rough else []) +
                                ([os.path.join(ROOT, "include", "svgf_highlight.h"), LIB_HIGHLIGHT] if shine else [])):
            continue
        tmp = out + f".tmp{os.getpid()}"
        _run([hipcc_path(), "--offload-arch=gfx950", "-O2", "-I", os.path.join(ROOT, "include"), src, "-L", _HERE] + (["-lsvgf_highlight"] if shine else []) + (["-lsvgf_rough"] if rough else []) + (["-lsvgf_virtual"] if virt else []) + (["-lsvgf_gloss"] if gloss else []) + (["-lsvgf_path"] if path else []) + (["-lsvgf_split"] if split else []) + (["-lsvgf_trace"] if traced else []) + ["-lsvgf_hip",
              "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN/../cuda-path-tracer-denoising_amd", "-o", tmp])
        os.replace(tmp, out)
    return out
