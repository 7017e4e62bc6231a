"""binding.py's surface, pinned by two golden files that were recorded before its repeated jobs were folded into helpers.

tests/golden/binding_abi.json: the ctypes prototypes load_library() / load_lbvh_library() leave on every exported symbol, the signature of
every public callable, every Structure's fields and size, the public constants, the public names and the aliases.
tests/golden/binding_calls.json: what every public wrapper passes to the libraries.  A second copy of the package is imported under
another name while ctypes.CDLL hands out recorders for libsvgf_*.so, and a script calls every public function and method in each of its
forms (camera dict / SvgfCamera, pixel_length default / given, AoS / planar, stream int / object / None, ...) with every keyword moved
off its default; then once more with the libraries answering -5, for the messages.  Only public names are used.

`python tests/test_binding_surface.py --record` rewrites both files from the tree it runs in (it builds first)."""
import ctypes as C
import hashlib
import importlib.util
import inspect
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_ABI, GOLDEN_CALLS = os.path.join(GOLDEN, "binding_abi.json"), os.path.join(GOLDEN, "binding_calls.json")
CLASSES = ("Denoiser", "Scene", "SceneTree", "GlossTable", "RoughTable")
HOST = 1 << 20      # the script's device pointers and every count lie below, every host address above


def _public_callables(ns):
    """(name, callable) of the public functions / methods of a module or an instance, sorted."""
    return [(n, getattr(ns, n)) for n in sorted(dir(ns)) if not n.startswith("_") and (inspect.isfunction(getattr(ns, n)) or inspect.ismethod(getattr(ns, n)))]


def snapshot_abi(pkg, root):
    B = pkg.binding
    tname = lambda t: None if t is None else t.__name__      # noqa: E731
    public = [n for n in dir(B) if not n.startswith("_")]
    snap = {"functions": {}, "signatures": {}, "structures": {}, "constants": {}, "names": public}
    for lib, exports in ((B.load_library(), B.EXPORTS), (B.load_lbvh_library(), B.LBVH_EXPORTS)):
        for sym in exports:
            f = getattr(lib, sym)
            snap["functions"][sym] = {"argtypes": None if f.argtypes is None else [tname(t) for t in f.argtypes], "restype": tname(f.restype)}
    for n, f in _public_callables(B):
        if f.__module__ == B.__name__:
            snap["signatures"][n] = str(inspect.signature(f))
    for c in CLASSES:
        snap["signatures"][c] = str(inspect.signature(getattr(B, c)))
        for n, f in _public_callables(getattr(B, c)):
            snap["signatures"][f"{c}.{n}"] = str(inspect.signature(f))
    for n in public:
        v = getattr(B, n)
        if isinstance(v, type) and issubclass(v, C.Structure):
            snap["structures"][n] = {"fields": [[k, t.__name__] for k, t in v._fields_], "sizeof": C.sizeof(v)}
        elif isinstance(v, str):
            snap["constants"][n] = os.path.relpath(v, root) if os.path.isabs(v) else v
        elif isinstance(v, (int, tuple, list, np.dtype)):
            snap["constants"][n] = str(v) if isinstance(v, np.dtype) else v
    snap["aliases"] = {"Scene.draw_planar is Scene.draw": B.Scene.draw_planar is B.Scene.draw, "ResidentScene is Scene": B.ResidentScene is B.Scene,
                       "Denoiser.denoiseFree is Denoiser.free": B.Denoiser.denoiseFree is B.Denoiser.free}
    return json.loads(json.dumps(snap))      # tuples as the lists the file holds


# --- the recording stand-in for the libraries -------------------------------------------------------------------------------------
GEOMS_AT = {"svgf_scene_create": 1, "svgf_scene_render_mesh": 7, "svgf_scene_render_mesh_planar": 7, "svgf_scene_render": 7}


def _sha(p, nbytes):
    return "NULL" if p is None else hashlib.sha1(C.string_at(p, nbytes)).hexdigest()[:12]


def _host_arrays(name, a):
    """Hashes of the host arrays of a scene call, read back through the pointers with the counts of the same call."""
    o = GEOMS_AT[name]
    out = ["geoms=" + _sha(a[o], 156 * a[o + 1])]
    if name != "svgf_scene_render":
        ng, nt, ntex = a[o + 1], a[o + 6], a[o + 10]
        desc = np.frombuffer(C.string_at(a[o + 8], 12 * ntex), np.int32).reshape(-1, 3) if ntex else None
        texels = int(desc[-1, 0] + 3 * desc[-1, 1] * desc[-1, 2]) if ntex else 0
        sizes = {2: 4 * ng, 3: 96 * nt, 4: 4 * nt, 5: 12 * nt, 7: 4 * nt, 8: 12 * ntex, 9: texels}
        out += [f"{k}={_sha(a[o + i], n)}" for (i, n), k in zip(sizes.items(), "geom_ids tris tri_ids tri_albedo tri_tex tex_desc texels".split())]
    return out


def _norm(name, args):
    out = []
    for i, a in enumerate(args):
        if a is None or isinstance(a, (float, bytes)):
            out.append(repr(a))
        elif isinstance(a, int):
            out.append(str(a) if -HOST < a < HOST else "host")
        elif hasattr(a, "_obj"):                        # byref(x)
            out.append(f"&{type(a._obj).__name__}:{bytes(a._obj).hex()}")
        elif isinstance(a, C._Pointer):                 # array.ctypes.data_as(POINTER(T)): hashed where the next argument is its count
            n = args[i + 1] if i + 1 < len(args) and isinstance(args[i + 1], int) else 0
            out.append(f"{type(a).__name__}:{_sha(C.cast(a, C.c_void_p).value, n * C.sizeof(a._type_))}")
        else:                                           # a ctypes value: a handle, an array passed as a pointer
            out.append(f"{type(a).__name__}:{bytes(a).hex()}")
    return out + (_host_arrays(name, args) if name in GEOMS_AT else [])


class Recorder:
    """ctypes.CDLL's stand-in: libsvgf_<tag>.so becomes an object whose svgf_* attributes record their calls and answer `rc`."""

    def __init__(self):
        self.rc, self.log, self.handles, self.real = 0, [], 0x7000, C.CDLL

    def cdll(self, path, *a, **kw):
        base = os.path.basename(str(path))
        if not base.startswith("libsvgf_"):
            return self.real(path, *a, **kw)
        self.log.append("CDLL " + base)
        return _Lib(self, base[len("libsvgf_"):-len(".so")])


class _Lib:
    def __init__(self, rec, tag):
        self._rec, self._tag = rec, tag

    def __getattr__(self, name):
        if not name.startswith("svgf_") or (name.startswith("svgf_exp_") and self._tag != "hip_exp"):
            raise AttributeError(name)
        setattr(self, name, _Fn(self._rec, self._tag, name))
        return getattr(self, name)


class _Fn:
    argtypes, restype = None, C.c_int

    def __init__(self, rec, tag, name):
        self.rec, self.tag, self.name = rec, tag, name

    def __call__(self, *args):
        self.rec.log.append(f"{self.tag}:{self.name}({', '.join(_norm(self.name, args))})")
        for a in args:
            if isinstance(getattr(a, "_obj", None), C.c_void_p):      # an out handle
                a._obj.value = self.rec.handles = self.rec.handles + 0x100
        if self.name == "svgf_params_sizeof":
            return 80
        if self.name.endswith("_version"):
            return 9
        return b"stand-in error" if self.name == "svgf_last_error" else self.rec.rc


class _Tensor:
    def __init__(self, ptr, numel=0):
        self.data_ptr, self.is_contiguous, self.numel = (lambda: ptr), (lambda: True), (lambda: numel)


class _Stream:
    cuda_stream = 0x900


def _kwargs(fn, values):
    """Every parameter of `fn`: from `values` by name, else its default moved by an amount of its own (None stays None)."""
    kw = {}
    for i, (n, p) in enumerate(inspect.signature(fn).parameters.items(), 1):
        d = p.default
        if n in values:
            kw[n] = values[n]
        elif d is inspect.Parameter.empty:
            raise KeyError(f"{fn.__qualname__}: the script has no value for `{n}`")
        else:
            kw[n] = d if d is None else (not d) if isinstance(d, bool) else tuple(x + i / 8 for x in d) if isinstance(d, tuple) else d + (i if isinstance(d, int) else i / 8)
    return kw


def snapshot_calls(ge):
    rec, name, out = Recorder(), ge.PKG_NAME + "_recorded", {}
    C.CDLL = rec.cdll
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ge.PKG_DIR, "__init__.py"), submodule_search_locations=[ge.PKG_DIR])
        sys.modules[name] = mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _script(mod.binding, mod.scene, rec, out)
    finally:
        C.CDLL = rec.real
        for m in [m for m in sys.modules if m == name or m.startswith(name + ".")]:
            del sys.modules[m]
    return out


def _script(B, scene, rec, out):
    def call(label, fn, *a, **kw):
        start, raised = len(rec.log), None
        try:
            r = fn(*a, **kw)
        except Exception as e:      # noqa: BLE001
            r, raised = None, f"{type(e).__name__}: {e}"
        assert label not in out, label
        out[label] = {"lib": rec.log[start:], "raises": raised}
        return r

    def routed():
        B.use_experiments_library(True)
        try:
            B.synth_camera(1, False, 6, 4)
            B.Denoiser(6, 4)
        finally:
            B.use_experiments_library(False)

    call("load_library", B.load_library)
    call("load_library(experiments=True)", B.load_library, experiments=True)
    for n in [c.name for c in B.COMPANIONS] + ["lbvh"]:
        call(f"load_{n}_library", getattr(B, f"load_{n}_library"))
    rng = np.random.default_rng(5)
    cam_d = dict(right=(1, 0, 0.5), up=(0, 1, 0.25), view=(0, 0, -1), position=(0.5, 1.5, 2.5), fovy_deg=60.0)
    geoms = np.frombuffer(rng.integers(0, 255, 2 * 156, dtype=np.uint8).tobytes(), scene.SCENE_GEOM_DTYPE)
    mesh = dict(geoms=geoms, geom_ids=[3, 4], tris=rng.random((5, 3, 8), dtype=np.float32), tri_ids=[5, 5, 6, 6, 7], tri_albedo=rng.random((5, 3), dtype=np.float32))
    textures = [rng.integers(0, 255, (2, 3, 3), dtype=np.uint8), rng.integers(0, 255, (4, 1, 3), dtype=np.uint8)]
    d = call("Denoiser", B.Denoiser, 6, 4, device=1)
    d2 = call("Denoiser(pipelined=True)", B.Denoiser, 6, 4, pipelined=True)
    dx = call("Denoiser(experiments=True)", B.Denoiser, 6, 4, 2, experiments=True)
    sc = call("Scene.create", B.Scene.create, **mesh, tri_tex=[0, -1, 1, 1, 0], textures=textures, max_leaf_tris=2, split=1, device=1)
    call("Scene.create(no geometry)", B.Scene.create, None, None, None, None, None)
    tree = call("SceneTree.create", B.SceneTree.create, sc, 2)
    gloss = call("GlossTable", B.GlossTable, rng.random((3, 6), dtype=np.float32).view(scene.SURFACE_DTYPE), device=1)
    rough = call("RoughTable", B.RoughTable, [0.25, 0.5], device=1)
    empty = [call("GlossTable(None)", B.GlossTable), call("RoughTable(None)", B.RoughTable, None)]
    call("len", lambda: (len(gloss), len(rough)))
    params, cam_s = B.reference_defaults().set(sigma_l=0.75, atrous_nlevel=3), B.SvgfCamera.from_dict(cam_d)
    # a value per parameter name: device pointers, raw and as tensors in turn; then the rest
    ptrs = ("out inp gbuffer out_rgb out_gbuffer out_direct out_indirect out_chain pbo left right state rgb a b se_map ssim_map exposure_state "
            "motion_out position geom_id normal albedo rgb_lo direct indirect guide_or_gbuffer nodes order").split()
    pool = {n: 0x1000 * k if k % 2 else _Tensor(0x1000 * k) for k, n in enumerate(ptrs, 1)}
    pool.update(mesh, width=6, height=4, W=6, H=4, width_hi=12, height_hi=8, width_lo=6, height_lo=4, frame=7, moving=True, step=2, kernel="lane",
                name="knob", value=3, path="frame.png", src=d2, scene=sc, which=2, n=2, nframes=5, k=2, slot=1, radius=2, rank=3, alpha=0.25,
                n_objects=3, sigma_n=0.5, sigma_x=0.75, modulate=1, axis=(0, 1, 0), angle_rad=0.5, stream_a=0x900, stream_b=_Stream(),
                planes=B.SvgfPlanarGBuffer(0xA1000, 0xA2000, 0xA3000, 0xA4000), geom_xf=_Tensor(0x51000, 36), tri_boxes=np.zeros(3, B.BVH_NODE_DTYPE),
                light=B.SvgfSceneLight.make((1, 2, 3), (0.5, 0, 0), (0, 0, 0.25), 4), hi_guide=B.guide(normal=0x61000, position=0x62000, geom_id=0x63000, albedo=0x64000),
                lo_guide=B.guide(gbuffer=_Tensor(0x65000)))
    forms = [dict(camera=cam_d, prev_camera=cam_d, pixel_length=None, stream=0x900, table=gloss, rough=rough, motion=None, params=None, tri_tex=[1, 1, -1, 0, 0],
                  textures=textures),
             dict(camera=cam_s, prev_camera=cam_s, pixel_length=(0.5, 0.25), stream=_Stream(), table=None, rough=None,
                  motion=_Tensor(0x52000), params=params, out_gbuffer=pool["planes"], tri_tex=None, textures=None, hi_guide=0x66000, lo_guide=_Tensor(0x67000),
                  guide_or_gbuffer=pool["lo_guide"], geom_xf=None),
             dict(stream=None), dict(camera=cam_s)]      # the last two: the first form on the default stream; a SvgfCamera without a pixel_length
    point, aos = dict(light=(1.0, 2.0, 3.0)), dict(out_gbuffer=pool["out_gbuffer"])      # the light as a point; the producers without a planar form
    special = {"save_png": dict(rgb=rng.random((4, 6, 3), dtype=np.float32)), "bvh_refit_plan_host": dict(nodes=np.zeros(3, B.BVH_NODE_DTYPE)),
               "Denoiser.denoise_host": dict(color=rng.random((4, 6, 3), dtype=np.float32), gbuffer=np.zeros(52 * 24, np.uint8), motion=None),
               "Scene.pose": dict(table=_Tensor(0x53000)), "Scene.draw": point, "Scene.draw_planar": point, "synth_render": aos, "scene_render": [dict(light=None, **aos), dict(point, **aos)],
               "scene_render_mesh": [dict(light=None), point]}
    # torch.cuda inside; the loaders, the switch and the frees have calls of their own here
    skip = {"exposure_state", "quality_state", "load_library", "use_experiments_library", "Denoiser.free", "Denoiser.denoiseFree", "Scene.free", "SceneTree.free",
            "Scene.create", "SceneTree.create"} | {f"load_{c}_library" for c in [c.name for c in B.COMPANIONS] + ["lbvh"]}
    targets = [(n, f) for n, f in _public_callables(B) if f.__module__ == B.__name__]
    targets += [(f"{type(o).__name__}.{n}", f) for o in (d, sc, tree) for n, f in _public_callables(o)]
    for rec.rc in (0, -5):
        for label, fn in targets:
            for k, form in enumerate(forms if rec.rc == 0 else forms[:1]):
                if label in skip or (k and not set(form) & set(inspect.signature(fn).parameters)) or (label, form.get("stream", 0)) == ("scene_render_mesh", None):
                    continue
                sp = special.get(label, {})
                call(f"{label} form {k} rc {rec.rc}", fn, **_kwargs(fn, {**pool, **forms[0], **form, **(sp[min(k, 1)] if isinstance(sp, list) else sp)}))
        call(f"Denoiser(experiments=True).level_kernels rc {rec.rc}", dx.level_kernels)
        call(f"use_experiments_library routes rc {rec.rc}", routed)
        for label, fn, a in (("Denoiser", B.Denoiser, (6, 4)), ("Scene.create", B.Scene.create, (None,) * 5), ("SceneTree.create", B.SceneTree.create, (sc,)),
                             ("GlossTable", B.GlossTable, ()), ("RoughTable", B.RoughTable, ())) if rec.rc else ():
            call(f"{label} rc {rec.rc}", fn, *a)
    call("free", lambda: [o.free() for o in (d, d2, dx, tree, sc, gloss, rough, *empty)] + [d.denoiseFree(), sc.free()])
    exp = B.load_library(experiments=True)
    out["experiments prototypes"] = {n: [t.__name__ for t in f.argtypes] for n, f in sorted(vars(exp).items()) if n.startswith("svgf_exp_") and f.argtypes is not None}


def _compare(want, got):
    for section in want:
        if isinstance(want[section], dict):
            assert set(got[section]) == set(want[section]), section
            for key in want[section]:
                assert got[section][key] == want[section][key], (section, key)
    assert got == want


def test_prototypes_signatures_structures_constants_and_names_are_the_recorded_ones(pkg):
    from conftest import ROOT
    want, got = json.load(open(GOLDEN_ABI)), snapshot_abi(pkg, ROOT)
    assert len(want["functions"]) == len(pkg.binding.EXPORTS) + len(pkg.binding.LBVH_EXPORTS) and all(want["aliases"].values())
    assert set(got["names"]) >= set(want["names"]), "a public name went away"
    assert set(got["names"]) == set(want["names"]), "a new name of binding.py is public"
    _compare(want, got)


def test_every_wrapper_passes_the_libraries_what_it_did(pkg):
    from conftest import ge
    want, got = json.load(open(GOLDEN_CALLS)), snapshot_calls(ge)
    assert len(want) > 200 and sum(bool(v["raises"]) for v in want.values() if "raises" in v) > 80
    _compare({"calls": want}, {"calls": got})


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import ROOT, ge
    ge.build()
    for path, snap in ((GOLDEN_ABI, snapshot_abi(ge.load_package(), ROOT)), (GOLDEN_CALLS, snapshot_calls(ge))):
        json.dump(snap, open(path, "w"), indent=1, sort_keys=True)
        print("wrote", path)
