"""The path-traced resident scene (include/svgf_trace.h row f17: svgf_trace_draw of libsvgf_trace.so, svgf_scene_view of the product).

The yardstick is tests/scene_trace_model.py: scene_model.render's first hit, scene_shadow_model's shadow rays, then the header's
bounce as a brute force over every primitive and triangle, float32 with the kernel's nesting.  Both sides perform the same operations
in the same order without contraction, and the nearest hit does not depend on the tree, so there is no tolerance to choose: colour
and every G-buffer field are compared on bits (NaNs in the same place count as equal), expected and allowed number of differing
pixels: 0.

CPU part: the accessor and the export lists; the sampler's statistics; bounce_samples = 0 against the shadowed model; the furnace;
colour bleeding; every `alt` of the model acts; the (pixel, sample) bounce rays on which the gate changes the hit are counted; and
what examples/traced_scene.cpp measures, on the oracle.  GPU part: the device against the model.

The sampler's bands.  d.n of a cosine-weighted direction has mean 2/3 and variance 1/2 - 4/9 = 1/18; a pixel whose four pairs all
miss the disc (probability q = (1 - pi/4)^4) takes the normal itself, d.n = 1.  So over N pixels the mean of d.n has expectation
2/3 + q/3 and standard error at most sqrt(1/18 / N) + the binomial share's, and the count of fallbacks is binomial(N, q).
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import scene_model as sm
import scene_pose_model as pm
import scene_shadow_model as ssm
import scene_trace_model as stm
import test_animated_scene as tas
import test_resident_scene as trs
import test_scene_model as tsm
import test_shadowed_scene as tss
from conftest import ROOT
from test_scene_model import FRAME, SEED, counts

F = np.float32
BUILDS = trs.BUILDS
SIZES = tss.SIZES
EDGE = tss.EDGE


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _furnace():
    """A sphere and a cube of albedo 1 that do not emit, inside an emitting cube of albedo 0.5 and emittance 2, the camera inside; the
    light's centre so far away that 4 + dist2 overflows and the light's term is exactly 0 everywhere.  With ambient = 1 every bounce
    brings back exactly 1: the enclosure 0.5 * 2, the two objects 1 * (1 + 0)."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = (0, 0, 0)
    geoms = tsm._geoms(pkg, (0, (0, 0, 0), z, (10, 10, 10), (0.5, 0.5, 0.5), 2.0), (1, (-1.2, -0.3, 0), z, (2, 2, 2), (1, 1, 1), 0.0),
                       (0, (1.4, 0.2, -0.5), (0, 30, 15), (1.5, 1.5, 1.5), (1, 1, 1), 0.0))
    s = dict(cam=tsm._cam(pkg, (0, 0.4, 2.6), (0, 0, 0), 40.0), geoms=geoms, geom_ids=None, tris=None, tri_ids=None, tri_albedo=None,
             tri_tex=None, textures=None, light=(0.0, 1e20, 0.0))
    return s, dict(centre=s["light"], edge_u=(0.0, 0.0, 0.0), edge_v=(0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def _bleed():
    """A white floor, a red wall standing on it at x = -3 and a white back wall; the light above the middle of the floor."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    z = (0, 0, 0)
    geoms = tsm._geoms(pkg, (0, (0, -0.1, 0), z, (12, 0.2, 12), (0.9, 0.9, 0.9), 0.0), (0, (-3.1, 3, 0), z, (0.2, 6, 12), (0.9, 0.1, 0.1), 0.0),
                       (0, (0, 3, -6.1), z, (12, 6, 0.2), (0.9, 0.9, 0.9), 0.0))
    s = dict(cam=tsm._cam(pkg, (1.5, 5, 9), (0, 0, 0), 40.0), geoms=geoms, geom_ids=None, tris=None, tri_ids=None, tri_albedo=None,
             tri_tex=None, textures=None, light=(0.0, 6.0, 0.0))
    return s, dict(centre=s["light"], edge_u=(0.5, 0.0, 0.0), edge_v=(0.0, 0.0, 0.5))


@functools.lru_cache(maxsize=None)
def _graze():
    """The scene on which the GATE decides bounce hits, after tss._graze.  A wall and an occluder (both windings) lie in ONE plane,
    turned out of the axes, and the wall's vertex normals lie IN that plane, towards the occluder.  Almost every bounce leaves the
    plane; the fallback direction of the rejection sampler (a = b = 0, two pixels in a thousand) is the normal itself and runs within
    rounding of the plane of all four triangles, where the float32 test accepts hits that lie nowhere near the triangle."""
    import __graft_entry__ as ge
    from temporal_harness import rotation
    pkg = ge.load_package()
    R = rotation("x", 25.0) @ rotation("y", -35.0)
    P = lambda x, y, z=0.0: tuple(float(c) for c in R @ np.array([x, y, z], np.float64))      # noqa: E731
    nrm = np.array([P(1, 0, 0)] * 3, F)
    tris = [tsm._tri(P(-4, -3), P(2, -3), P(-4, 3), nrm=nrm), tsm._tri(P(2, -3), P(2, 3), P(-4, 3), nrm=nrm, k=1),
            tsm._tri(P(3, -1.5), P(4.5, 0), P(3, 1.5), k=2), tsm._tri(P(3, -1.5), P(3, 1.5), P(4.5, 0), k=3)]
    s = dict(cam=tsm._cam(pkg, P(-1, 0, 5), P(-1, 0, 0), 25.0), geoms=tsm._geoms(pkg), geom_ids=None, tris=np.stack(tris),
             tri_ids=np.array([1, 1, 2, 3], np.int32), tri_albedo=tsm._colours(4, 9), tri_tex=None, textures=None, light=P(0, 0, 6))
    return s, dict(centre=s["light"], edge_u=P(0.3, 0, 0), edge_v=P(0, 0.3, 0))


@functools.lru_cache(maxsize=None)
def _textured_floor():
    """Scene C's textured quads (in the plane z = 0, facing the camera) and a floor primitive under them that reaches towards the
    camera: half of its bounce goes back and up, onto the textured triangles."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    s = tsm._scene("C")
    P = np.asarray(s["tris"], F).reshape(-1, 3, 8)[:, :, :3].reshape(-1, 3)
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    e = float((hi - lo).max())
    slab = (0, (0.0, lo[1] - 0.02 * e, 0.25 * e), (0, 0, 0), (e, 0.02 * e, 0.5 * e), (0.8, 0.8, 0.8), 0.0)
    s = tss._add(pkg, s, geoms=[slab])
    return s, dict(centre=tuple(s["light"]), edge_u=(0.2, 0, 0), edge_v=(0, 0.2, 0))


def _input(kind, name):
    if kind == "traced":
        return {"furnace": _furnace, "bleed": _bleed, "graze": _graze, "textured": _textured_floor}[name]()
    return tss._input(kind, name)


@functools.lru_cache(maxsize=None)
def _first(kind, name, W, H, frame, seed, noise=0.6):
    if kind != "traced":
        return tss._first(kind, name, W, H, frame, seed, noise)
    s = _input(kind, name)[0]
    first = sm.render(W, H, frame, *tss._args(s), s["light"], seed=seed, noise=noise, fireflies=0.02 if noise else 0.0)
    em = ssm.emitter_mask(W, H, s["cam"], s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"])
    for a in first + (em,):
        a.setflags(write=False)
    return first, em


@functools.lru_cache(maxsize=None)
def _model(kind, name, W, H, J, sec=1, samples=1, point=False, alt=None, frame=FRAME, seed=SEED, noise=0.6, ambient=0.15):
    s, lk = _input(kind, name)
    lt = ssm.light(lk["centre"], samples=samples) if point else ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    first, em = _first(kind, name, W, H, frame, seed, noise)
    col, gb, info = stm.render(W, H, frame, *tss._args(s), lt, stm.params(J, ambient, sec), seed=seed, noise=noise, fireflies=0.02 if noise else 0.0,
                               alt=alt, first=first, emitters=em)
    col.setflags(write=False)
    return (col, gb), info, lt


def _no_difference(got, ref, what):
    c = counts(got, ref)
    print(f"{what}: differing pixels {c} (expected and allowed: 0)")
    assert not any(c.values()), f"{what}: {c}"


# ---- CPU 1: the accessor and the two export lists --------------------------------------------------------------------------------------
def test_the_accessor_and_the_companion_librarys_exports(pkg):
    lib, B = pkg.load_library(), pkg.binding
    v = B.SvgfSceneView()
    assert lib.svgf_scene_view(None, ctypes.byref(v)) == -1 and lib.svgf_scene_view(None, None) == -1
    assert ctypes.sizeof(B.SvgfSceneView) == 112 and ctypes.sizeof(B.SvgfTraceParams) == 12 and B.TRACE_MAX_BOUNCE_SAMPLES == 8
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgf_trace.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(svgf_trace_[a-z_]+)\s*\(", src)))
    assert declared == sorted(B.TRACE_EXPORTS) and len(declared) == 2
    path = B.LIB_TRACE_PATH
    assert os.path.exists(path), "libsvgf_trace.so is built by __graft_entry__.build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert set(B.TRACE_EXPORTS) <= exported and not any(n.startswith("svgf_") and n not in B.TRACE_EXPORTS for n in exported)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "svgf_scene_view" in undefined and "getenv" not in undefined
    needed = subprocess.run(["readelf", "-d", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libsvgf_hip.so" in needed
    print(f"libsvgf_hip.so {os.path.getsize(B.LIB_PATH)} bytes, libsvgf_trace.so {os.path.getsize(path)} bytes")


def test_trace_argument_errors_without_a_device(pkg):
    B = pkg.binding
    lib = pkg.load_trace_library()
    assert lib.svgf_trace_version() == pkg.load_library().svgf_version()
    cam, sp, planes = B.SvgfCamera(), B.SvgfSynthParams(), B.SvgfPlanarGBuffer()
    ok, tp = B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4), B.SvgfTraceParams(1, 0.15, 1)
    call = lambda lt, tp, gb=1, pl=None: lib.svgf_trace_draw(None, 1, gb, pl, 8, 8, ctypes.byref(cam), ctypes.byref(sp), lt, tp, None)  # noqa: E731
    assert call(None, ctypes.byref(tp)) == -1 and call(ctypes.byref(ok), None) == -1 and call(ctypes.byref(ok), ctypes.byref(tp)) == -1
    for n in (0, -1, 65):
        assert call(ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), samples=n)), ctypes.byref(tp)) == -1, n
    assert call(ctypes.byref(ok), ctypes.byref(tp), gb=1, pl=ctypes.byref(planes)) == -1 and call(ctypes.byref(ok), ctypes.byref(tp), gb=None) == -1


# ---- CPU 2: the sampler ---------------------------------------------------------------------------------------------------------------
def _ulps(x, ref):
    return np.abs(x.astype(np.float64) - ref) / np.spacing(F(ref)).astype(np.float64)


def test_the_frame_is_orthonormal():
    """Hashed normals and the poles, -0.0 included: T, B and n are orthonormal to 8 ulp of 1 (no branch, no singularity at n.z = -1
    for copysign picks the other chart there)."""
    N = 1 << 12
    v = [(F(2.0) * stm.synth.hash_uniform(5, 2, N, k) - F(1.0)).astype(F) for k in range(3)]
    n = stm._normalise(v)
    poles = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0.0], [1, 0, -0.0], [0, -1, 0.0], [0, 1, -0.0], [0.6, 0.8, -0.0], [1e-20, 0, -1], [0, 1e-7, 1]], F)
    n = [np.concatenate([n[c], poles[:, c]]) for c in range(3)]
    T, B = stm.frame_of(n)
    d64 = lambda a, b: sum(a[c].astype(np.float64) * b[c].astype(np.float64) for c in range(3))        # noqa: E731
    eps = 8 * float(np.spacing(F(1.0)))
    worst = max(np.abs(d64(T, T) - 1).max(), np.abs(d64(B, B) - 1).max(), np.abs(d64(T, B)).max(), np.abs(d64(T, n)).max(), np.abs(d64(B, n)).max())
    print(f"{len(n[0])} normals: worst deviation from orthonormal {worst:.3e} (allowed {eps:.3e})")
    assert np.isfinite(T).all() and np.isfinite(B).all() and worst <= eps


def test_the_sampler_is_cosine_weighted_and_the_fallback_is_rare():
    N = 1 << 16
    v = [(F(2.0) * stm.synth.hash_uniform(9, 4, N, k) - F(1.0)).astype(F) for k in range(3)]
    n = stm._normalise(v)
    d, fb = stm.directions(11, 3, N, np.arange(N), n, 1)
    d, fb = [d[c][0] for c in range(3)], fb[0]
    length = np.sqrt(sum(d[c].astype(np.float64) ** 2 for c in range(3)))
    dn = sum(d[c].astype(np.float64) * n[c].astype(np.float64) for c in range(3))
    q = (1.0 - np.pi / 4.0) ** 4
    share, s_share = fb.mean(), np.sqrt(q * (1 - q) / N)
    mean, want = dn.mean(), 2.0 / 3.0 + q / 3.0
    se = np.sqrt(1.0 / 18.0 / N) + s_share / 3.0
    print(f"{N} pixels: |d| - 1 worst {np.abs(length - 1).max():.3e}, min d.n {dn.min():.3e}, mean d.n {mean:.5f} (expected {want:.5f} +- {se:.5f}), "
          f"fallback share {share:.5f} (expected {q:.5f} +- {s_share:.5f})")
    assert np.abs(length - 1).max() <= 4 * float(np.spacing(F(1.0))) and dn.min() >= -2.0 ** -22
    assert abs(mean - want) <= 4 * se and abs(share - q) <= 4 * s_share
    assert (dn[fb] > 1 - 1e-6).all()


# ---- CPU 3: the model's own properties -------------------------------------------------------------------------------------------------
def test_no_bounce_and_the_stub_ambient_give_the_shadowed_models_frame():
    for kind, name in (("edge", "B"), ("edge", "E_plus"), ("made", "stage"), ("plain", "D")):
        W, H = 67, 41
        (col, gb), info, lt = _model(kind, name, W, H, 0, samples=3)
        ref = tss._model(kind, name, W, H, 3)[0]
        _no_difference((col, gb), ref, f"{name}: bounce_samples 0, ambient 0.15 vs scene_shadow_model")


@pytest.mark.parametrize("J", [1, 3, 8])
def test_the_furnace_returns_exactly_one(J):
    W, H = 48, 27
    (col, gb), info, _ = _model("traced", "furnace", W, H, J, noise=0.0, ambient=1.0)
    cast = info["cast"]
    ind = info["ind"][cast]
    print(f"furnace, {J} samples: {int(cast.sum())} pixels bounce, {int(info['hit'].sum())} of {info['hit'].size} rays hit, "
          f"{int(info['emitter_hit'].sum())} the enclosure; ind in [{ind.min()}, {ind.max()}]")
    assert cast.sum() > 200 and info["hit"].all() and info["emitter_hit"].any() and not info["emitter_hit"].all()
    assert (ind == F(1.0)).all()
    want = (gb["albedo"] * F(2.0)).astype(F)            # ((alb * ((1 + vis * 0) + 1)) * 1) * 1
    assert not tsm.differing(col, want)[cast].any()
    em = _first("traced", "furnace", W, H, FRAME, SEED, 0.0)[1]
    assert em.sum() > 200 and (col[em] == F(1.0)).all()                    # the enclosure itself: 0.5 * 2


def test_colour_bleeds_from_the_red_wall_onto_the_floor():
    W, H, J = 48, 27, 8
    (col, gb), info, _ = _model("traced", "bleed", W, H, J, noise=0.0)
    x, ind = gb["position"][..., 0], info["ind"].astype(np.float64)
    floor = gb["geomId"] == 0
    near, far = floor & (x < -2.0), floor & (x > 1.0)
    ratio = lambda m: ind[m][:, 0].sum() / ind[m][:, 1].sum()           # noqa: E731
    print(f"bleed: {int(near.sum())} floor pixels within one unit of the wall, red / green of the indirect term {ratio(near):.3f}; "
          f"{int(far.sum())} pixels four units away and more: {ratio(far):.3f}")
    assert near.sum() > 20 and far.sum() > 100
    assert ratio(near) > 1.0 and ratio(far) < ratio(near)


ALT_SCENES = [("edge", n, 67, 41, 3) for n in EDGE] + [("made", "stage", 67, 41, 3), ("traced", "furnace", 67, 41, 3), ("traced", "graze", 200, 120, 8)]


def test_each_alt_acts():
    """Pixels on which the frame of the model and of a wrong variant of it differ, per scene (the bounce's shadow ray on): every alt
    changes some scene.  `ungated` needs the grazing scene, and there the fallback rays: 200x120 with 8 bounce samples."""
    total = {a: 0 for a in stm.ALTS}
    for kind, name, W, H, J in ALT_SCENES:
        ref = _model(kind, name, W, H, J)[0]
        row = {}
        for alt in stm.ALTS:
            row[alt] = tsm.any_differs(_model(kind, name, W, H, J, alt=alt)[0], ref)
            total[alt] += row[alt]
        print(f"scene {name} {W}x{H}, {J} bounce samples: {row}")
    print(f"all scenes: {total}")
    for alt, n in total.items():
        assert n > 0, f"`{alt}` changes no pixel of any scene"


GATE_ZERO = [("edge", "A", 3), ("edge", "B", 3), ("edge", "F_cube", 3), ("edge", "F_sphere", 3), ("edge", "E_plus", 3), ("rec", "cornell", 3),
             ("rec", "room", 1)]


def test_the_gate_decides_bounce_hits_of_the_grazing_scene():
    """The one scene here on which it is NOT zero: made for it, see _graze."""
    W, H, J = 200, 120, 8
    info = _model("traced", "graze", W, H, J)[1]
    print(f"graze {W}x{H}, {J} bounce samples: {info['hit'].size} rays, {int(info['fallback'].sum())} of them the fallback, {int(info['hit'].sum())} hit, "
          f"the gate changes {info['ungated_differs']}")
    assert info["ungated_differs"] > 0


@pytest.mark.parametrize("kind,name,J", GATE_ZERO)
def test_the_gate_changes_no_bounce_hit(kind, name, J):
    """(pixel, sample) bounce rays whose nearest triangle differs between the contract and an ungated brute force."""
    W, H = {"cornell": (96, 96), "room": (128, 72)}.get(name, (67, 41))
    info = _model(kind, name, W, H, J, frame=0 if kind == "rec" else FRAME, seed=1 if kind == "rec" else SEED)[1]
    print(f"{name} {W}x{H}, {J} bounce samples: {info['hit'].size} rays, {int(info['hit'].sum())} hit, the gate changes {info['ungated_differs']}")
    assert info["hit"].any() and info["ungated_differs"] == 0


# ---- CPU 4: what examples/traced_scene.cpp measures, on the oracle ---------------------------------------------------------------------
def test_denoised_bounce_beats_the_noisy_one_after_eight_static_frames(pkg, orc):
    """64x36, noise 0 (the one-sample bounce and the one-sample shadow are the only noise), eight frames of the example's room with the
    block at rest through the oracle's full SVGF, against the model's converged frame: 8 bounce samples x 64 shadow rays averaged over
    16 frame seeds.  The gate is the issue's: the denoised frame beats the noisy one in PSNR and in mean SSIM.  Recorded on the last
    frame: noisy 11.23 dB / SSIM 0.5195, denoised 19.72 dB / SSIM 0.6600 (a bounce that finds the light's slab brings back five times
    the image's white: the noisy frame is mostly fireflies).  The first scene tried; not a law."""
    import quality_model as qm
    from temporal_harness import scales
    W, H, N = 64, 36, 8
    geoms, cam, lk = tss._example_scene()
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, W, H)
    first = sm.render(W, H, 0, cam, geoms, None, None, None, None, None, None, lk["centre"], seed=7, noise=0.0, fireflies=0.0)
    em = ssm.emitter_mask(W, H, cam, geoms, None, None, None)
    frame = lambda f, J, samples: stm.render(W, H, f, cam, geoms, None, None, None, None, None, None, ssm.light(samples=samples, **lk),   # noqa: E731
                                             stm.params(J, 0.15, 1), seed=7, noise=0.0, fireflies=0.0, first=first, emitters=em)
    o = orc.Oracle(pkg, W, H, threads=4)
    try:
        for f in range(N):
            noisy, gb, _ = frame(f, 1, 1)
            out = o.denoise(noisy, gb, cam, p).reshape(H, W, 3)
    finally:
        o.free()
    ref = np.mean([frame(100 + k, 8, 64)[0].astype(np.float64) for k in range(16)], axis=0).astype(F)
    qn, qd = qm.meter(noisy, ref), qm.meter(out, ref)
    print(f"frame {N - 1}: noisy {qn['psnr_db']:.2f} dB / SSIM {qn['mean_ssim']:.4f}, denoised {qd['psnr_db']:.2f} dB / SSIM {qd['mean_ssim']:.4f}")
    assert qd["psnr_db"] > qn["psnr_db"] and qd["mean_ssim"] > qn["mean_ssim"]


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def _draw(pkg, scene, W, H, s, lt, J, sec=1, ambient=0.15, frame=FRAME, seed=SEED, noise=0.6, stream=None, bufs=None, sync=True):
    import torch
    rgb, gbt = bufs or trs._buffers(W, H)
    light = pkg.binding.SvgfSceneLight.make(lt["centre"], lt["edge_u"], lt["edge_v"], lt["samples"])
    scene.draw_traced(rgb, gbt, W, H, s["cam"], light, frame, bounce_samples=J, ambient=ambient, shadow_secondary=sec, seed=seed, noise=noise,
                      fireflies=0.02 if noise else 0.0, stream=stream)
    if not sync:
        return None
    torch.cuda.synchronize()
    return trs._host(pkg, rgb, gbt, W, H)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_sizes_and_seams(pkg, W, H):
    s = tss._edge("B")[0]
    scene = trs._create(pkg, s)
    ref, info, lt = _model("edge", "B", W, H, 3, samples=2)
    got = _draw(pkg, scene, W, H, s, lt, 3)
    scene.free()
    _no_difference(got, ref, f"scene B {W}x{H}, 3 bounce samples")


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_edge_scene_with_an_occluder_equals_the_model(pkg, name):
    W, H = 67, 41
    s = tss._edge(name)[0]
    scene = trs._create(pkg, s)
    hits = 0
    for J in (1, 3, 8):
        for sec in (0, 1):
            for point in (True, False):
                ref, info, lt = _model("edge", name, W, H, J, sec, samples=1, point=point)
                hits += int(info["hit"].sum())
                _no_difference(_draw(pkg, scene, W, H, s, lt, J, sec), ref,
                               f"scene {name}, {J} bounce samples, secondary shadow {sec}, {'point' if point else 'area'} light")
    scene.free()
    assert hits > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,J", [("cornell", 96, 96, 3), ("room", 128, 72, 1)])
def test_recorded_scene_equals_the_model(pkg, name, W, H, J):
    s = trs._recorded(name, 0)[0]
    scene = trs._create(pkg, s)
    ref, info, lt = _model("rec", name, W, H, J, frame=0, seed=1)
    got = _draw(pkg, scene, W, H, s, lt, J, frame=0, seed=1)
    scene.free()
    print(f"{name}: {int(info['hit'].sum())} of {info['hit'].size} bounce rays hit, {int(info['secondary_occluded'].sum())} of them shadowed")
    _no_difference(got, ref, f"{name} {W}x{H}, {J} bounce samples")


@pytest.mark.gpu
@pytest.mark.parametrize("J", [1, 3, 8])
def test_the_furnace_on_the_device(pkg, J):
    W, H = 48, 27
    s = _furnace()[0]
    ref, info, lt = _model("traced", "furnace", W, H, J, noise=0.0, ambient=1.0)
    scene = trs._create(pkg, s)
    got = _draw(pkg, scene, W, H, s, lt, J, ambient=1.0, noise=0.0)
    scene.free()
    _no_difference(got, ref, f"furnace, {J} bounce samples")
    assert (got[0][info["cast"]] == (got[1]["albedo"][info["cast"]] * F(2.0)).astype(F)).all()


@pytest.mark.gpu
def test_nan_normals_textures_and_made_scenes_equal_the_model(pkg):
    """Scene D (a mesh without normals: NaN directions miss), scenes C and G, the stage (emitters met by the bounce), f16's grazing
    scene, colour bleeding, and the bounce's own grazing scene, where the gate decides hits."""
    for kind, name, W, H, J in (("plain", "D", 67, 41, 3), ("plain", "C", 67, 41, 3), ("plain", "G", 67, 41, 3), ("made", "stage", 67, 41, 3),
                                ("made", "graze", 67, 41, 3), ("traced", "bleed", 67, 41, 3), ("traced", "graze", 200, 120, 8)):
        s = _input(kind, name)[0]
        scene = trs._create(pkg, s)
        ref, info, lt = _model(kind, name, W, H, J, samples=2)
        _no_difference(_draw(pkg, scene, W, H, s, lt, J), ref, f"{name} {W}x{H}, {J} bounce samples")
        scene.free()


@pytest.mark.gpu
def test_a_textured_mesh_at_the_secondary_hit(pkg):
    """_textured_floor: the model says how many bounce rays end on a textured triangle, and the device agrees on every bit."""
    W, H = 67, 41
    s, lk = _textured_floor()
    scene = trs._create(pkg, s)
    ref, info, lt = _model("traced", "textured", W, H, 3, samples=1)
    tex_ids = set(np.asarray(s["tri_ids"])[np.asarray(s["tri_tex"]) >= 0].tolist())
    on_texture = int(np.isin(info["hit_gid"], list(tex_ids)).sum())
    print(f"{on_texture} of {info['hit'].size} bounce rays end on a textured triangle")
    assert on_texture > 100
    _no_difference(_draw(pkg, scene, W, H, s, lt, 3), ref, "textured mesh at the secondary hit")
    scene.free()


@pytest.mark.gpu
def test_planar_target_equals_the_model(pkg):
    import torch
    from temporal_harness import _hip
    W, H = 67, 41
    s = tss._edge("F_cube")[0]
    ref, _, lt = _model("edge", "F_cube", W, H, 3, samples=2)
    scene = trs._create(pkg, s)
    den = pkg.Denoiser(W, H, 0)
    planes = den.planar_gbuffer()
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    scene.draw_traced(rgb, planes, W, H, s["cam"], pkg.binding.SvgfSceneLight.make(lt["centre"], lt["edge_u"], lt["edge_v"], 2), FRAME, bounce_samples=3,
                      seed=SEED)
    torch.cuda.synchronize()
    hip = _hip()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    gb = np.zeros((H, W), dtype=pkg.synth.GBUFFER_DTYPE)
    for field, ptr in (("normal", planes.normal), ("position", planes.position), ("albedo", planes.albedo), ("geomId", planes.geom_id)):
        host = np.zeros((H, W, 3) if field != "geomId" else (H, W), F if field != "geomId" else np.int32)
        assert hip.hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0
        gb[field] = host
    gb["ialbedo"] = F(1.0)
    got = (rgb.cpu().numpy(), gb)
    den.free(); scene.free()
    _no_difference(got, ref, "scene F_cube, planar target")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "cornell"])
def test_every_tree_draws_the_same_traced_frame(pkg, name):
    (kind, W, H, J, fr, sd) = ("edge", 67, 41, 3, FRAME, SEED) if name == "A" else ("rec", 96, 96, 3, 0, 1)
    s = _input(kind, name)[0]
    ref, _, lt = _model(kind, name, W, H, J, frame=fr, seed=sd)
    for ml, sp in BUILDS:
        scene = trs._create(pkg, s, ml, sp)
        got = _draw(pkg, scene, W, H, s, lt, J, frame=fr, seed=sd)
        scene.free()
        _no_difference(got, ref, f"{name}, leaf {ml} split {sp}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "E_plus"])
def test_no_bounce_is_svgf_scene_draw_shadowed_on_bits(pkg, name):
    W, H = 67, 41
    s = tss._edge(name)[0]
    scene = trs._create(pkg, s)
    lt = tss._model("edge", name, W, H, 3)[2]
    got = _draw(pkg, scene, W, H, s, lt, 0)
    shadowed = tss._draw(pkg, scene, W, H, s, lt)
    scene.free()
    _no_difference(got, shadowed, f"scene {name}: bounce_samples 0, ambient 0.15 vs svgf_scene_draw_shadowed")


@functools.lru_cache(maxsize=None)
def _block_frame(f, W, H, J, samples=1, noise=0.6):
    """Frame f of f15's turning block under f16's area light: the model on the posed arrays."""
    s, tables = tas._block_inputs()
    ps = pm.posed_scene(s, tables[f])
    lk = tss._block_light()
    lt = ssm.light(lk["centre"], lk["edge_u"], lk["edge_v"], samples)
    col, gb, info = stm.render(W, H, f, ps["cam"], ps["geoms"], None, None, None, None, None, None, lt, stm.params(J), seed=3, noise=noise,
                               fireflies=0.02 if noise else 0.0)
    return (col, gb), info, lt


@pytest.mark.gpu
def test_the_bounce_follows_the_pose_and_the_view_moves_to_the_posed_arrays(pkg):
    W, H = 96, 96
    s, tables = tas._block_inputs()
    scene = trs._create(pkg, s)
    before = scene.view()
    info_ = scene.info()
    assert before["n_geoms"] == info_["n_geoms"] == len(s["geoms"]) and before["n_tris"] == 0 and before["depth"] == info_["depth"]
    assert before["device"] == 0 and before["geoms"] != 0 and before["geom_ids"] == 0 and before["tri_tex"] == 0
    assert scene.view() == before                                       # a pure accessor
    scene.enable_pose(len(s["geoms"]))
    after = scene.view()
    assert after["geoms"] != before["geoms"] and after["nodes"] != before["nodes"] and after["tris"] != before["tris"]
    assert after["tri_boxes"] != before["tri_boxes"] and after["order"] == before["order"] and after["tex"] == before["tex"]
    ind = []
    for f in (0, 2):
        ref, info, lt = _block_frame(f, W, H, 2)
        scene.pose(tas._dev(tables[f]))
        _no_difference(_draw(pkg, scene, W, H, s, lt, 2, frame=f, seed=3), ref, f"turning block, pose {f}")
        ind.append(info["ind"])
    assert scene.view() == after
    scene.free()
    assert int((ind[0] != ind[1]).any(axis=-1).sum()) > 50


@pytest.mark.gpu
def test_eight_traced_draws_queued_without_host_waits(pkg):
    import torch
    W, H = 67, 41
    s = tss._edge("A")[0]
    scene = trs._create(pkg, s)
    st = torch.cuda.Stream()
    bufs = [trs._buffers(W, H) for _ in range(8)]
    lt = _model("edge", "A", W, H, 2)[2]
    for f, b in enumerate(bufs):
        _draw(pkg, scene, W, H, s, lt, 2, frame=f, stream=st, bufs=b, sync=False)
    st.synchronize()
    for f, (rgb, gbt) in enumerate(bufs):
        _no_difference(trs._host(pkg, rgb, gbt, W, H), _model("edge", "A", W, H, 2, frame=f)[0], f"queued draw, frame {f}")
    scene.free()


@pytest.mark.gpu
def test_a_captured_traced_draw_is_one_kernel_node_and_replays_the_same_bits(pkg):
    import torch
    hip = tas._graph_api()
    W, H = 67, 41
    s = tss._edge("B")[0]
    ref, _, lt = _model("edge", "B", W, H, 3)
    scene = trs._create(pkg, s)
    st = torch.cuda.Stream()
    bufs = trs._buffers(W, H)
    _draw(pkg, scene, W, H, s, lt, 3, stream=st, bufs=bufs, sync=False)       # eager first: a first launch may set kernel attributes
    st.synchronize()
    graph, gexec = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamBeginCapture(st.cuda_stream, 2) == 0
    _draw(pkg, scene, W, H, s, lt, 3, stream=st, bufs=bufs, sync=False)       # recorded, not executed
    assert hip.hipStreamEndCapture(st.cuda_stream, ctypes.byref(graph)) == 0 and graph.value
    types = tas._node_types(hip, graph)
    assert hip.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0) == 0
    with torch.cuda.stream(st):
        bufs[0].zero_(); bufs[1].zero_()
    assert hip.hipGraphLaunch(gexec, st.cuda_stream) == 0
    st.synchronize()
    got = trs._host(pkg, *bufs, W, H)
    hip.hipGraphExecDestroy(gexec); hip.hipGraphDestroy(graph)
    scene.free()
    print(f"captured traced draw = node types {types}")
    assert types == [0], types
    _no_difference(got, ref, "replayed traced draw")


@pytest.mark.gpu
def test_every_error_code(pkg):
    B = pkg.binding
    s = tss._edge("B")[0]
    scene = trs._create(pkg, s)
    lib = pkg.load_trace_library()
    cam, sp, planes = B.SvgfCamera(), B.SvgfSynthParams(), B.SvgfPlanarGBuffer()
    ok = ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4))
    tp = ctypes.byref(B.SvgfTraceParams(1, 0.15, 1))
    c, p = ctypes.byref(cam), ctypes.byref(sp)
    f = lib.svgf_trace_draw
    assert f(scene.h, 1, 1, None, 0, 8, c, p, ok, tp, None) == -1 and f(scene.h, 1, 1, None, 8, -1, c, p, ok, tp, None) == -1
    assert f(scene.h, None, 1, None, 8, 8, c, p, ok, tp, None) == -1 and f(scene.h, 1, None, None, 8, 8, c, p, ok, tp, None) == -1
    assert f(scene.h, 1, 1, None, 8, 8, None, p, ok, tp, None) == -1 and f(scene.h, 1, 1, None, 8, 8, c, None, ok, tp, None) == -1
    assert f(scene.h, 1, 1, None, 8, 8, c, p, None, tp, None) == -1 and f(None, 1, 1, None, 8, 8, c, p, ok, tp, None) == -1
    assert f(scene.h, 1, 1, ctypes.byref(planes), 8, 8, c, p, ok, tp, None) == -1        # both targets
    assert f(scene.h, 1, None, ctypes.byref(planes), 8, 8, c, p, ok, tp, None) == -1     # planes without normal, position, geom_id
    assert f(scene.h, 1, 1, None, 1 << 14, 1 << 13, c, p, ok, tp, None) == -5            # width * height == 2^31 / 16
    for n in (0, 65):
        assert f(scene.h, 1, 1, None, 8, 8, c, p, ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), samples=n)), tp, None) == -1
    bad = B.SvgfSceneLight.make((0, 1, 0), samples=1)
    bad.edge_v[2] = float("nan")
    assert f(scene.h, 1, 1, None, 8, 8, c, p, ctypes.byref(bad), tp, None) == -1
    assert f(scene.h, 1, 1, None, 8, 8, c, p, ok, None, None) == -1                      # a NULL tp
    for J, amb, sec in ((-1, 0.15, 1), (9, 0.15, 1), (1, float("nan"), 1), (1, float("inf"), 1), (1, -0.5, 1), (1, 0.15, 2), (1, 0.15, -1)):
        assert f(scene.h, 1, 1, None, 8, 8, c, p, ok, ctypes.byref(B.SvgfTraceParams(J, amb, sec)), None) == -1, (J, amb, sec)
    v = B.SvgfSceneView()
    assert scene.lib.svgf_scene_view(scene.h, None) == -1 and scene.lib.svgf_scene_view(scene.h, ctypes.byref(v)) == 0
    assert v.n_tris == len(s["tris"]) and v.n_nodes == scene.info()["n_nodes"] and v.tris and v.nodes and v.order and v.tri_boxes
    # and the scene still draws
    W, H = 7, 5
    ref, _, lt = _model("edge", "B", W, H, 3)
    _no_difference(_draw(pkg, scene, W, H, s, lt, 3), ref, "after the refused calls")
    scene.free()


@pytest.mark.gpu
def test_pose_traced_draw_denoise_sequence(pkg, orc):
    """128x72, six frames of the turning block on one stream: pose -> traced draw (1 bounce sample, 1 shadow ray) -> svgf_denoise
    (temporal pass), with the object motion table, against tests/temporal_model.py fed the model's frames - with the f8 firefly filter
    off and on (tests/firefly_model.py filters the model's input the way the first pass does)."""
    import torch
    import firefly_model as fm
    import temporal_model as tm
    from temporal_harness import assert_frames_equal, read_states, scales, synth_params
    W, H = 128, 72
    s, tables = tas._block_inputs()
    n = len(s["geoms"])
    held, frames, motion = pkg.binding.pose_identity(n), [], []
    for f, t in enumerate(tables):
        (col, gb), _, lt = _block_frame(f, W, H, 1)
        frames.append((np.asarray(col, F).reshape(H, W, 3), gb.reshape(H, W)))
        motion.append(pm.motion_rows(held, t))
        held = t
    M = orc.view_matrix(pkg, s["cam"])
    p = synth_params(pkg, W, H)
    for rank, scale in ((0, 1.0), (2, 1.0)):
        fed = [(fm.firefly_filter(c, rank, scale), g) for c, g in frames]
        want = tm.run_sequence(fed, tables=motion, views=[M] * len(frames), scale=scales(pkg, W, H), radius=0, k=0.0)
        scene = trs._create(pkg, s)
        scene.enable_pose(n)
        den = pkg.Denoiser(W, H)
        den.set_capture(True)
        t_x = tas._motion_buffer(n)
        den.set_object_motion(t_x)
        den.set_firefly_filter(rank, scale)
        rgb, gbt = trs._buffers(W, H)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        got = []
        try:
            for f, t in enumerate(tables):
                scene.pose(tas._dev(t), t_x)
                _draw(pkg, scene, W, H, s, lt, 1, frame=f, seed=3, bufs=(rgb, gbt), sync=False)
                den.denoise(out, rgb, gbt, s["cam"], p)
                torch.cuda.synchronize()
                got.append(read_states(den))
        finally:
            den.free(); scene.free()
        assert_frames_equal(got, want, f"firefly filter rank {rank}")
