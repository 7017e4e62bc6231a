"""Build recipe of the product library (no cmake, no JIT cache): everything lands in-tree so it travels to the GPU box.
The checkers (CPU restatement, the reference's own denoise.cu) have their own recipe outside this package."""
from __future__ import annotations

import collections
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
# The companion libraries (renderer-side code beside the product library, which stays what it was: tests/test_abi.py caps its size), in
# the order they were added: the short name (libsvgf_<name>.so, include/svgf_<name>.h), the .hip sources, and the public headers it is
# compiled against besides svgf.h.  Each is a library of its own, linked against the product alone, so that the ones before it stay the
# code objects they were; the kernels are shared as text (csrc/svgf_scene_trace.inc.h, csrc/svgf_scene_gloss.inc.h).  binding.COMPANIONS
# is the loader's side of this table; DESIGN.md 5.4p says how a row is added.
Companion = collections.namedtuple("Companion", "name sources headers")
COMPANIONS = (
    Companion("trace", ["svgf_scene_trace.hip"], ["svgf_trace.h"]),                                                    # f17: one bounce
    Companion("split", ["svgf_scene_split.hip", "svgf_trace_compose.hip"], ["svgf_trace.h", "svgf_split.h"]),          # f18: D and I apart
    Companion("path", ["svgf_scene_path.hip"], ["svgf_trace.h", "svgf_path.h"]),                                       # f19: deep paths
    Companion("gloss", ["svgf_scene_gloss.hip"], ["svgf_trace.h", "svgf_path.h", "svgf_gloss.h"]),                     # f20: mirror, glass
    Companion("virtual", ["svgf_scene_virtual.hip"], ["svgf_trace.h", "svgf_path.h", "svgf_gloss.h", "svgf_virtual.h"]),   # f21: virtual hits
    Companion("rough", ["svgf_scene_rough.hip"], ["svgf_trace.h", "svgf_path.h", "svgf_gloss.h", "svgf_virtual.h", "svgf_rough.h"]),   # f22: GGX lobe
    Companion("highlight", ["svgf_scene_highlight.hip"],                                                               # f23: the light's GGX term
              ["svgf_trace.h", "svgf_path.h", "svgf_gloss.h", "svgf_virtual.h", "svgf_rough.h", "svgf_highlight.h"]),
)
# Libraries built by the companions' recipe that are no companion draw (no Scene.draw_* method, no example, not part of build_all()):
# the same row, and the flags the row's sources need on top of HIPCC_FLAGS.  Row f24's device BVH builder states its result as
# float32 arithmetic with one rounding per operation, in kernels and in the host builder alike: -ffp-contract=off.
Builder = collections.namedtuple("Builder", "name sources headers flags")
BUILDERS = (
    Builder("lbvh", ["svgf_lbvh.hip", "svgf_lbvh_host.cpp"], ["svgf_lbvh.h"], ["-ffp-contract=off"]),                  # f24: LBVH on the device
)
# Tree builders added after BUILDERS was pinned to row f24's: the same row type, the same recipe.  Row f25 restates svgf_bvh_build_host's
# float32 / double arithmetic on the device, one rounding per operation: -ffp-contract=off.
TREE_BUILDERS = (
    Builder("sah", ["svgf_sah.hip"], ["svgf_sah.h"], ["-ffp-contract=off"]),                                           # f25: binned SAH on the device
)
# Libraries that write the triangles the tree builders read, added after TREE_BUILDERS was pinned to row f25's: the same row type, the
# same recipe.  Row f26 states its skin as float32 arithmetic with one rounding per operation: -ffp-contract=off.
SCENE_WRITERS = (
    Builder("deform", ["svgf_deform.hip", "svgf_deform_rig.cpp"], ["svgf_deform.h", "svgf_scene_write.h"], ["-ffp-contract=off"]),   # f26: skinned triangles
)
# Libraries that light a G-buffer of the resident scene from a table of lights, added after SCENE_WRITERS was pinned to row f26's: the
# same row type, the same recipe.  Row f27 states its reservoirs as float32 arithmetic with one rounding per operation: -ffp-contract=off.
LIGHT_SAMPLERS = (
    Builder("restir", ["svgf_restir.hip"], ["svgf_restir.h"], ["-ffp-contract=off"]),                                  # f27: ReSTIR DI
)
# Libraries that resample the paths behind a G-buffer of the resident scene, added after LIGHT_SAMPLERS was pinned to row f27's: the same
# row type, the same recipe.  Row f28 states its reservoirs as float32 arithmetic with one rounding per operation: -ffp-contract=off.
PATH_RESAMPLERS = (
    Builder("restir_gi", ["svgf_restir_gi.hip"], ["svgf_restir_gi.h", "svgf_trace.h"], ["-ffp-contract=off"]),         # f28: ReSTIR GI
)


def companion_path(name: str) -> str:
    return os.path.join(_HERE, f"libsvgf_{name}.so")


LIB_TRACE, LIB_SPLIT, LIB_PATH, LIB_GLOSS, LIB_VIRTUAL, LIB_ROUGH, LIB_HIGHLIGHT = (companion_path(c.name) for c in COMPANIONS)
TRACE_SOURCES, SPLIT_SOURCES, PATH_SOURCES, GLOSS_SOURCES, VIRTUAL_SOURCES, ROUGH_SOURCES, HIGHLIGHT_SOURCES = (c.sources for c in COMPANIONS)
# examples/<name>.cpp -> the companions it links, in link order (every example links the product library behind them).  Row f26's, row f27's and row f28's
# stand in directories of their own: the list of examples/*.cpp is pinned (tests/golden/companion_abi.json).
EXAMPLES = {"pipeline": (), "farm": (), "cadence": (), "upsample": (), "dynres": (), "hdr_display": (), "quality": (), "resident_scene": (),
            "animated_scene": (), "shadowed_scene": (), "traced_scene": ("trace",), "split_scene": ("split", "trace"),
            "path_scene": ("path", "split"), "gloss_scene": ("gloss", "split"), "virtual_scene": ("virtual", "gloss", "split"),
            "rough_scene": ("rough", "gloss", "split"), "highlight_scene": ("highlight", "rough", "gloss", "split"),
            "deform/deform_scene": ("deform", "sah"), "restir/restir_scene": ("restir", "split"),
            "restir_gi/restir_gi_scene": ("restir_gi", "restir", "split")}
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


def _jobs() -> int:
    """Width of the compile pool: MAX_JOBS where it is set, else the host's CPUs, 16 at the most (a shared host shows more than a build may use)."""
    return max(1, int(os.environ.get("MAX_JOBS") or min(16, os.cpu_count() or 1)))


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
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(srcs), _jobs())) as pool:
            list(pool.map(lambda so: _run([hipcc_path()] + (CXX_FLAGS if os.path.basename(so[0]) in CXX_SOURCES else
                                                            cflags + HIPCC_FILE_FLAGS.get(os.path.basename(so[0]), []) + extra) + ["-c", so[0], "-o", so[1]]),
                          zip(srcs, objs)))
        # the product library is linked stripped (-Wl,-s: host side, link line only): .symtab / .strtab go, the dynamic symbols and
        # the device code objects (.dynsym, .hip_fatbin) stay; DESIGN.md 5.4g has the sizes with and without
        _run([hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC"] + ([] if experiments else ["-Wl,-s"]) + objs + ["-o", tmp])
    os.replace(tmp, LIB)              # atomic: concurrent ranks never see a half-written library
    return LIB


def build_companion(name: str, force: bool = False) -> str:
    """Compile the sources of COMPANIONS' (or BUILDERS' / TREE_BUILDERS' / SCENE_WRITERS' / LIGHT_SAMPLERS' / PATH_RESAMPLERS') row `name` for gfx950 into cuda-path-tracer-denoising_amd/libsvgf_<name>.so, linked against
    the product library beside it and against no other companion (the examples' rpath scheme: the build directory, then $ORIGIN, so the
    pair can be moved together)."""
    build_hip()
    c = next(c for c in COMPANIONS + BUILDERS + TREE_BUILDERS + SCENE_WRITERS + LIGHT_SAMPLERS + PATH_RESAMPLERS if c.name == name)
    lib = companion_path(name)
    srcs = [os.path.join(CSRC, s) for s in c.sources]
    deps = srcs + [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
        [os.path.join(ROOT, "include", h) for h in ["svgf.h"] + c.headers] + [LIB]
    if not force and _newer(lib, deps):
        return lib
    tmp = lib + f".tmp{os.getpid()}"
    _run([hipcc_path()] + HIPCC_FLAGS + list(getattr(c, "flags", [])) + srcs + ["-L", _HERE, "-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN", "-Wl,-s", "-o", tmp])
    os.replace(tmp, lib)
    return lib


def build_trace(force: bool = False) -> str:
    return build_companion("trace", force)


def build_split(force: bool = False) -> str:
    return build_companion("split", force)


def build_path(force: bool = False) -> str:
    return build_companion("path", force)


def build_gloss(force: bool = False) -> str:
    return build_companion("gloss", force)


def build_virtual(force: bool = False) -> str:
    return build_companion("virtual", force)


def build_rough(force: bool = False) -> str:
    return build_companion("rough", force)


def build_highlight(force: bool = False) -> str:
    return build_companion("highlight", force)


def build_lbvh(force: bool = False) -> str:
    """libsvgf_lbvh.so (row f24, include/svgf_lbvh.h): BUILDERS' row through the companions' recipe."""
    return build_companion("lbvh", force)


def build_sah(force: bool = False) -> str:
    """libsvgf_sah.so (row f25, include/svgf_sah.h): TREE_BUILDERS' row through the companions' recipe."""
    return build_companion("sah", force)


def build_deform(force: bool = False) -> str:
    """libsvgf_deform.so (row f26, include/svgf_deform.h): SCENE_WRITERS' row through the companions' recipe."""
    return build_companion("deform", force)


def build_restir(force: bool = False) -> str:
    """libsvgf_restir.so (row f27, include/svgf_restir.h): LIGHT_SAMPLERS' row through the companions' recipe."""
    return build_companion("restir", force)


def build_restir_gi(force: bool = False) -> str:
    """libsvgf_restir_gi.so (row f28, include/svgf_restir_gi.h): PATH_RESAMPLERS' row through the companions' recipe."""
    return build_companion("restir_gi", force)


def build_all(force: bool = False) -> list[str]:
    """The product library and the seven companion libraries, in the order they were added."""
    return [build_hip(force)] + [build_companion(c.name, force) for c in COMPANIONS]


def build_examples(force: bool = False) -> str:
    """Compile every examples/<name>.cpp of EXAMPLES through the C ABI into examples/<name>, linked in-tree against the companions its row
    names and the product library (each example's header comment says what it shows).  Returns the last one's path."""
    for c in COMPANIONS:
        build_companion(c.name)
    rows = COMPANIONS + BUILDERS + TREE_BUILDERS + SCENE_WRITERS + LIGHT_SAMPLERS + PATH_RESAMPLERS
    for name in sorted({n for links in EXAMPLES.values() for n in links} - {c.name for c in COMPANIONS}):
        build_companion(name)
    out = ""
    for name, links in EXAMPLES.items():
        src = os.path.join(ROOT, "examples", name + ".cpp")
        out = os.path.join(ROOT, "examples", name)
        deps = [src, os.path.join(ROOT, "include", "svgf.h"), LIB] + [companion_path(n) for n in links] + \
            [os.path.join(ROOT, "include", h) for c in rows if c.name in links for h in c.headers]
        if not force and _newer(out, deps):
            continue
        tmp = out + f".tmp{os.getpid()}"
        _run([hipcc_path(), "--offload-arch=gfx950", "-O2", "-I", os.path.join(ROOT, "include"), src, "-L", _HERE] + [f"-lsvgf_{n}" for n in links] +
             ["-lsvgf_hip", "-Wl,-rpath," + _HERE, "-Wl,-rpath,$ORIGIN/" + "../" * (1 + name.count("/")) + "cuda-path-tracer-denoising_amd", "-o", tmp])
        os.replace(tmp, out)
    return out
