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
import os
import re
import subprocess

import numpy as np
import pytest

import scene_harness as sh
import scene_model as sm
import scene_shadow_model as ssm
import scene_trace_model as stm
import test_scene_model as tsm
from conftest import ROOT
from test_scene_model import FRAME, SEED

F = np.float32


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
        (col, gb), info, lt = sh.traced_model(kind, name, W, H, 0, samples=3)
        ref = sh.shadow_model(kind, name, W, H, 3)[0]
        sh.same((col, gb), ref, f"{name}: bounce_samples 0, ambient 0.15 vs scene_shadow_model")


@pytest.mark.parametrize("J", [1, 3, 8])
def test_the_furnace_returns_exactly_one(J):
    W, H = 48, 27
    (col, gb), info, _ = sh.traced_model("traced", "furnace", W, H, J, noise=0.0, ambient=1.0)
    cast = info["cast"]
    ind = info["ind"][cast]
    print(f"furnace, {J} samples: {int(cast.sum())} pixels bounce, {int(info['hit'].sum())} of {info['hit'].size} rays hit, "
          f"{int(info['emitter_hit'].sum())} the enclosure; ind in [{ind.min()}, {ind.max()}]")
    assert cast.sum() > 200 and info["hit"].all() and info["emitter_hit"].any() and not info["emitter_hit"].all()
    assert (ind == F(1.0)).all()
    want = (gb["albedo"] * F(2.0)).astype(F)            # ((alb * ((1 + vis * 0) + 1)) * 1) * 1
    assert not tsm.differing(col, want)[cast].any()
    em = sh.first_hit("traced", "furnace", W, H, FRAME, SEED, 0.0)[1]
    assert em.sum() > 200 and (col[em] == F(1.0)).all()                    # the enclosure itself: 0.5 * 2


def test_colour_bleeds_from_the_red_wall_onto_the_floor():
    W, H, J = 48, 27, 8
    (col, gb), info, _ = sh.traced_model("traced", "bleed", W, H, J, noise=0.0)
    x, ind = gb["position"][..., 0], info["ind"].astype(np.float64)
    floor = gb["geomId"] == 0
    near, far = floor & (x < -2.0), floor & (x > 1.0)
    ratio = lambda m: ind[m][:, 0].sum() / ind[m][:, 1].sum()           # noqa: E731
    print(f"bleed: {int(near.sum())} floor pixels within one unit of the wall, red / green of the indirect term {ratio(near):.3f}; "
          f"{int(far.sum())} pixels four units away and more: {ratio(far):.3f}")
    assert near.sum() > 20 and far.sum() > 100
    assert ratio(near) > 1.0 and ratio(far) < ratio(near)


ALT_SCENES = [("edge", n, 67, 41, 3) for n in sh.EDGE] + [("made", "stage", 67, 41, 3), ("traced", "furnace", 67, 41, 3), ("traced", "graze", 200, 120, 8)]


def test_each_alt_acts():
    """Pixels on which the frame of the model and of a wrong variant of it differ, per scene (the bounce's shadow ray on): every alt
    changes some scene.  `ungated` needs the grazing scene, and there the fallback rays: 200x120 with 8 bounce samples."""
    total = {a: 0 for a in stm.ALTS}
    for kind, name, W, H, J in ALT_SCENES:
        ref = sh.traced_model(kind, name, W, H, J)[0]
        row = {}
        for alt in stm.ALTS:
            row[alt] = tsm.any_differs(sh.traced_model(kind, name, W, H, J, alt=alt)[0], ref)
            total[alt] += row[alt]
        print(f"scene {name} {W}x{H}, {J} bounce samples: {row}")
    print(f"all scenes: {total}")
    for alt, n in total.items():
        assert n > 0, f"`{alt}` changes no pixel of any scene"


GATE_ZERO = [("edge", "A", 3), ("edge", "B", 3), ("edge", "F_cube", 3), ("edge", "F_sphere", 3), ("edge", "E_plus", 3), ("rec", "cornell", 3),
             ("rec", "room", 1)]


def test_the_gate_decides_bounce_hits_of_the_grazing_scene():
    """The one scene here on which it is NOT zero: made for it, see scene_harness._graze_bounce."""
    W, H, J = 200, 120, 8
    info = sh.traced_model("traced", "graze", W, H, J)[1]
    print(f"graze {W}x{H}, {J} bounce samples: {info['hit'].size} rays, {int(info['fallback'].sum())} of them the fallback, {int(info['hit'].sum())} hit, "
          f"the gate changes {info['ungated_differs']}")
    assert info["ungated_differs"] > 0


@pytest.mark.parametrize("kind,name,J", GATE_ZERO)
def test_the_gate_changes_no_bounce_hit(kind, name, J):
    """(pixel, sample) bounce rays whose nearest triangle differs between the contract and an ungated brute force."""
    W, H = {"cornell": (96, 96), "room": (128, 72)}.get(name, (67, 41))
    info = sh.traced_model(kind, name, W, H, J, frame=0 if kind == "rec" else FRAME, seed=1 if kind == "rec" else SEED)[1]
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
    geoms, cam, lk = sh.example_scene()
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
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", sh.SIZES)
def test_sizes_and_seams(pkg, W, H):
    s = sh.edge("B")[0]
    scene = sh.create(pkg, s)
    ref, info, lt = sh.traced_model("edge", "B", W, H, 3, samples=2)
    got = sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(3))
    scene.free()
    sh.same(got, ref, f"scene B {W}x{H}, 3 bounce samples")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sh.EDGE)
def test_edge_scene_with_an_occluder_equals_the_model(pkg, name):
    W, H = 67, 41
    s = sh.edge(name)[0]
    scene = sh.create(pkg, s)
    hits = 0
    for J in (1, 3, 8):
        for sec in (0, 1):
            for point in (True, False):
                ref, info, lt = sh.traced_model("edge", name, W, H, J, sec, samples=1, point=point)
                hits += int(info["hit"].sum())
                sh.same(sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(J, sec)), ref,
                               f"scene {name}, {J} bounce samples, secondary shadow {sec}, {'point' if point else 'area'} light")
    scene.free()
    assert hits > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,J", [("cornell", 96, 96, 3), ("room", 128, 72, 1)])
def test_recorded_scene_equals_the_model(pkg, name, W, H, J):
    s = sh.recorded(name, 0)[0]
    scene = sh.create(pkg, s)
    ref, info, lt = sh.traced_model("rec", name, W, H, J, frame=0, seed=1)
    got = sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(J), frame=0, seed=1)
    scene.free()
    print(f"{name}: {int(info['hit'].sum())} of {info['hit'].size} bounce rays hit, {int(info['secondary_occluded'].sum())} of them shadowed")
    sh.same(got, ref, f"{name} {W}x{H}, {J} bounce samples")


@pytest.mark.gpu
@pytest.mark.parametrize("J", [1, 3, 8])
def test_the_furnace_on_the_device(pkg, J):
    W, H = 48, 27
    s = sh.furnace()[0]
    ref, info, lt = sh.traced_model("traced", "furnace", W, H, J, noise=0.0, ambient=1.0)
    scene = sh.create(pkg, s)
    got = sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(J, ambient=1.0, noise=0.0))
    scene.free()
    sh.same(got, ref, f"furnace, {J} bounce samples")
    assert (got["color"][info["cast"]] == (got["gb"]["albedo"][info["cast"]] * F(2.0)).astype(F)).all()


@pytest.mark.gpu
def test_nan_normals_textures_and_made_scenes_equal_the_model(pkg):
    """Scene D (a mesh without normals: NaN directions miss), scenes C and G, the stage (emitters met by the bounce), f16's grazing
    scene, colour bleeding, and the bounce's own grazing scene, where the gate decides hits."""
    for kind, name, W, H, J in (("plain", "D", 67, 41, 3), ("plain", "C", 67, 41, 3), ("plain", "G", 67, 41, 3), ("made", "stage", 67, 41, 3),
                                ("made", "graze", 67, 41, 3), ("traced", "bleed", 67, 41, 3), ("traced", "graze", 200, 120, 8)):
        s = sh.scene_input(kind, name)[0]
        scene = sh.create(pkg, s)
        ref, info, lt = sh.traced_model(kind, name, W, H, J, samples=2)
        sh.same(sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(J)), ref, f"{name} {W}x{H}, {J} bounce samples")
        scene.free()


@pytest.mark.gpu
def test_a_textured_mesh_at_the_secondary_hit(pkg):
    """scene_harness.textured_floor: the model says how many bounce rays end on a textured triangle, and the device agrees on every bit."""
    W, H = 67, 41
    s, lk = sh.textured_floor()
    scene = sh.create(pkg, s)
    ref, info, lt = sh.traced_model("traced", "textured", W, H, 3, samples=1)
    tex_ids = set(np.asarray(s["tri_ids"])[np.asarray(s["tri_tex"]) >= 0].tolist())
    on_texture = int(np.isin(info["hit_gid"], list(tex_ids)).sum())
    print(f"{on_texture} of {info['hit'].size} bounce rays end on a textured triangle")
    assert on_texture > 100
    sh.same(sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(3)), ref, "textured mesh at the secondary hit")
    scene.free()


@pytest.mark.gpu
def test_planar_target_equals_the_model(pkg):
    W, H = 67, 41
    s = sh.edge("F_cube")[0]
    ref, _, lt = sh.traced_model("edge", "F_cube", W, H, 3, samples=2)
    sh.check_planar_target(pkg, sh.TRACED, sh.case(s, W, H, lt, sh.trace_args(3)), ref, "scene F_cube, planar target")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "cornell"])
def test_every_tree_draws_the_same_traced_frame(pkg, name):
    (kind, W, H, J, fr, sd) = ("edge", 67, 41, 3, FRAME, SEED) if name == "A" else ("rec", 96, 96, 3, 0, 1)
    s = sh.scene_input(kind, name)[0]
    ref, _, lt = sh.traced_model(kind, name, W, H, J, frame=fr, seed=sd)
    sh.check_every_tree(pkg, sh.TRACED, sh.case(s, W, H, lt, sh.trace_args(J), fr, sd), ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B", "E_plus"])
def test_no_bounce_is_svgf_scene_draw_shadowed_on_bits(pkg, name):
    W, H = 67, 41
    s = sh.edge(name)[0]
    scene = sh.create(pkg, s)
    lt = sh.shadow_model("edge", name, W, H, 3)[2]
    got = sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(0))
    shadowed = sh.draw(pkg, sh.SHADOWED, scene, W, H, s, lt)
    scene.free()
    sh.same(got, shadowed, f"scene {name}: bounce_samples 0, ambient 0.15 vs svgf_scene_draw_shadowed")


@pytest.mark.gpu
def test_the_bounce_follows_the_pose_and_the_view_moves_to_the_posed_arrays(pkg):
    W, H = 96, 96
    s, tables = sh.block_inputs()
    scene = sh.create(pkg, s)
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
        ref, info, lt = sh.traced_block_frame(f, W, H, 2)
        scene.pose(sh.dev(tables[f]))
        sh.same(sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(2), frame=f, seed=3), ref, f"turning block, pose {f}")
        ind.append(info["ind"])
    assert scene.view() == after
    scene.free()
    assert int((ind[0] != ind[1]).any(axis=-1).sum()) > 50


@pytest.mark.gpu
def test_eight_traced_draws_queued_without_host_waits(pkg):
    W, H = 67, 41
    lt = sh.traced_model("edge", "A", W, H, 2)[2]
    sh.check_queued(pkg, sh.TRACED, sh.case(sh.edge("A")[0], W, H, lt, sh.trace_args(2)), lambda f: sh.traced_model("edge", "A", W, H, 2, frame=f)[0],
                    "queued draw", own_stream=False)


@pytest.mark.gpu
def test_a_captured_traced_draw_is_one_kernel_node_and_replays_the_same_bits(pkg):
    W, H = 67, 41
    ref, _, lt = sh.traced_model("edge", "B", W, H, 3)
    sh.check_captured(pkg, sh.TRACED, sh.case(sh.edge("B")[0], W, H, lt, sh.trace_args(3)), ref, "traced draw", own_stream=False)


@pytest.mark.gpu
def test_every_error_code(pkg):
    B = pkg.binding
    s = sh.edge("B")[0]
    scene = sh.create(pkg, s)
    lib = pkg.load_trace_library()
    c, p = ctypes.byref(B.SvgfCamera()), ctypes.byref(B.SvgfSynthParams())
    ok = ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4))
    tp = ctypes.byref(B.SvgfTraceParams(1, 0.15, 1))
    f = lambda h=scene.h, rgb=1, gb=1, pl=None, w=8, hh=8, cm=c, spp=p, lt=ok, t=tp: lib.svgf_trace_draw(h, rgb, gb, pl, w, hh, cm, spp, lt, t, None)  # noqa: E731
    assert f(rgb=None) == -1
    sh.check_common_refusals(B, f, (B.SvgfTraceParams, sh.BAD_TRACE))
    v = B.SvgfSceneView()
    assert scene.lib.svgf_scene_view(scene.h, None) == -1 and scene.lib.svgf_scene_view(scene.h, ctypes.byref(v)) == 0
    assert v.n_tris == len(s["tris"]) and v.n_nodes == scene.info()["n_nodes"] and v.tris and v.nodes and v.order and v.tri_boxes
    # and the scene still draws
    W, H = 7, 5
    ref, _, lt = sh.traced_model("edge", "B", W, H, 3)
    sh.same(sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(3)), ref, "after the refused calls")
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
    s, tables = sh.block_inputs()
    n = len(s["geoms"])
    frames, motion = [], sh.block_motion(pkg, tables)
    for f in range(len(tables)):
        (col, gb), _, lt = sh.traced_block_frame(f, W, H, 1)
        frames.append((np.asarray(col, F).reshape(H, W, 3), gb.reshape(H, W)))
    M = orc.view_matrix(pkg, s["cam"])
    p = synth_params(pkg, W, H)
    for rank, scale in ((0, 1.0), (2, 1.0)):
        fed = [(fm.firefly_filter(c, rank, scale), g) for c, g in frames]
        want = tm.run_sequence(fed, tables=motion, views=[M] * len(frames), scale=scales(pkg, W, H), radius=0, k=0.0)
        scene = sh.create(pkg, s)
        scene.enable_pose(n)
        den = pkg.Denoiser(W, H)
        den.set_capture(True)
        t_x = sh.motion_buffer(n)
        den.set_object_motion(t_x)
        den.set_firefly_filter(rank, scale)
        rgb, gbt = sh.buffers(W, H)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        got = []
        try:
            for f, t in enumerate(tables):
                scene.pose(sh.dev(t), t_x)
                sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(1), frame=f, seed=3, bufs=dict(color=rgb, gb=gbt), sync=False)
                den.denoise(out, rgb, gbt, s["cam"], p)
                torch.cuda.synchronize()
                got.append(read_states(den))
        finally:
            den.free(); scene.free()
        assert_frames_equal(got, want, f"firefly filter rank {rank}")
