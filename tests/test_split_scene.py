"""The split traced scene (include/svgf_split.h row f18, libsvgf_split.so): svgf_trace_draw_split writes direct and indirect light apart and without the
albedo, svgf_trace_compose puts two (denoised) terms back together.

The yardstick is tests/scene_split_model.py on top of tests/scene_trace_model.py.  The draw performs the model's operations in the
model's order without contraction, so D, I, the colour and every G-buffer field are compared on bits (NaNs in the same place count as
equal): expected and allowed number of differing pixels 0.  The recomposition is one addition and one multiplication: bits again.

The one bound in this file, compose(alb, D, I) against svgf_trace_draw's colour, is derived: see
test_the_recomposed_frame_is_the_traced_frame_up_to_rounding.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import scene_harness as sh
import scene_model as sm
import scene_pose_model as pm
import scene_shadow_model as ssm
import scene_split_model as spm
import scene_trace_model as stm
from conftest import ROOT
from test_scene_model import FRAME, SEED, differing

F = np.float32


# ---- CPU 1: exports and refusals -------------------------------------------------------------------------------------------------------
def test_both_symbols_are_declared_listed_and_exported(pkg):
    """libsvgf_split.so exports what include/svgf_split.h declares and SPLIT_EXPORTS lists; libsvgf_trace.so and the product library
    export what they exported (tests/test_traced_scene.py pins the former to its two functions)."""
    B = pkg.binding
    assert sorted(B.SPLIT_EXPORTS) == ["svgf_trace_compose", "svgf_trace_draw_split"] and not set(B.SPLIT_EXPORTS) & set(B.TRACE_EXPORTS)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgf_split.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(svgf_[a-z_]+)\s*\(", src))
    assert declared == set(B.SPLIT_EXPORTS)
    nm = lambda path, how: subprocess.run(["nm", "-D", how, path], stdout=subprocess.PIPE, text=True, check=True).stdout      # noqa: E731
    exported = {ln.split()[-1] for ln in nm(B.LIB_SPLIT_PATH, "--defined-only").splitlines() if ln.strip()}
    assert set(B.SPLIT_EXPORTS) <= exported and not any(n.startswith("svgf_") and n not in B.SPLIT_EXPORTS for n in exported)
    undefined = nm(B.LIB_SPLIT_PATH, "--undefined-only")
    assert "svgf_scene_view" in undefined and "getenv" not in undefined and "svgf_trace_draw" not in undefined
    needed = subprocess.run(["readelf", "-d", B.LIB_SPLIT_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libsvgf_hip.so" in needed and "libsvgf_trace.so" not in needed
    for path, names in ((B.LIB_PATH, B.EXPORTS), (B.LIB_TRACE_PATH, B.TRACE_EXPORTS)):
        other = {ln.split()[-1] for ln in nm(path, "--defined-only").splitlines() if ln.strip()}
        assert set(names) <= other and not any("compose" in n or "split" in n for n in other)
    assert callable(pkg.trace_compose) and callable(pkg.Scene.draw_traced_split)
    print(f"libsvgf_trace.so {os.path.getsize(B.LIB_TRACE_PATH)} bytes, libsvgf_split.so {os.path.getsize(B.LIB_SPLIT_PATH)} bytes")


def test_split_draw_argument_errors_without_a_device(pkg):
    """Every refusal is answered before any device work: none of these calls needs a device (there is no scene without one, so the
    scene is NULL throughout, which is itself refused; the GPU test repeats the list with a scene)."""
    B = pkg.binding
    lib = pkg.load_split_library()
    cam, sp, planes = B.SvgfCamera(), B.SvgfSynthParams(), B.SvgfPlanarGBuffer()
    ok, tp = B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4), B.SvgfTraceParams(1, 0.15, 1)
    call = lambda lt, tp, d=1, i=2, rgb=3, gb=4, pl=None, w=8, h=8: lib.svgf_trace_draw_split(    # noqa: E731
        None, d, i, rgb, gb, pl, w, h, ctypes.byref(cam), ctypes.byref(sp), lt, tp, None)
    L, T = ctypes.byref(ok), ctypes.byref(tp)
    assert call(None, T) == -1 and call(L, None) == -1 and call(L, T) == -1
    for n in (0, -1, 65):
        assert call(ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), samples=n)), T) == -1, n
    assert call(L, T, pl=ctypes.byref(planes)) == -1 and call(L, T, gb=None) == -1
    assert call(L, T, d=None) == -1 and call(L, T, i=None) == -1 and call(L, T, d=5, i=5) == -1 and call(L, T, rgb=None) == -1
    assert call(L, T, w=0) == -1 and call(L, T, h=-3) == -1
    for J, amb, sec in ((-1, 0.15, 1), (9, 0.15, 1), (1, float("nan"), 1), (1, -0.5, 1), (1, 0.15, 2)):
        assert call(L, ctypes.byref(B.SvgfTraceParams(J, amb, sec))) == -1


def test_compose_argument_errors_without_a_device(pkg):
    B = pkg.binding
    f = pkg.load_split_library().svgf_trace_compose
    aos, planar, empty = B.guide(gbuffer=64), B.guide(albedo=64), B.guide(normal=64, position=64, geom_id=64)
    g = ctypes.byref(aos)
    assert f(0, None, 16, 32, g, 8, 8, None) == -1 and f(0, 48, None, 32, g, 8, 8, None) == -1 and f(0, 48, 16, None, g, 8, 8, None) == -1
    assert f(0, 48, 16, 32, None, 8, 8, None) == -1 and f(0, 48, 16, 32, ctypes.byref(empty), 8, 8, None) == -1
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -1)):
        assert f(0, 48, 16, 32, g, w, h, None) == -1 and f(0, 48, 16, 32, ctypes.byref(planar), w, h, None) == -1
    assert f(0, 48, 16, 32, g, 1 << 14, 1 << 13, None) == -5 and f(0, 48, 16, 32, ctypes.byref(planar), 1 << 27, 1, None) == -5
    assert f(1 << 20, 48, 16, 32, g, 8, 8, None) == -2           # no such device: refused, nothing launched


# ---- CPU 2: the model's own properties -------------------------------------------------------------------------------------------------
SMALL = [("edge", n, 67, 41) for n in sh.EDGE] + [("rec", "cornell", 96, 96)]


def _case(kind, name, W, H, J, **kw):
    rec = kind == "rec"
    return sh.split_model(kind, name, W, H, J, frame=0 if rec else FRAME, seed=1 if rec else SEED, **kw)


@pytest.mark.parametrize("kind,name,W,H", SMALL)
def test_without_noise_the_terms_are_the_shade_and_the_bounce(kind, name, W, H):
    m = _case(kind, name, W, H, 3, noise=0.0)
    info, gb = m["info"], m["gb"]
    cast, em, miss = info["cast"], info["emitter"], gb["geomId"] < 0
    print(f"{name}: {int(cast.sum())} pixels cast, {int(em.sum())} emitter pixels, {int(miss.sum())} misses")
    assert cast.sum() > 0
    for c in range(3):
        assert not differing(m["D"][..., c][..., None], info["shade0"][..., None])[cast].any()
    assert not differing(m["I"], info["ind"])[cast].any() and (info["ind"][cast] > 0).any()
    # an emitter: I = +0 and a * D is the traced colour on bits; a miss: both +0
    assert (m["I"].view(np.uint32)[em | miss] == 0).all() and (m["D"].view(np.uint32)[miss] == 0).all()
    aD = (gb["albedo"] * m["D"]).astype(F)
    assert not differing(aD, m["color"])[em].any()
    # no bounce: I is +0.0f everywhere, D unchanged
    z = _case(kind, name, W, H, 0, noise=0.0)
    assert (z["I"].view(np.uint32) == 0).all() and not differing(z["D"], m["D"]).any()


def test_the_stage_has_emitter_pixels_and_they_carry_no_indirect_light():
    m = sh.split_model("made", "stage", 67, 41, 3, noise=0.0)
    em = m["info"]["emitter"]
    print(f"stage: {int(em.sum())} emitter pixels")
    assert em.sum() >= 10 and (m["I"].view(np.uint32)[em] == 0).all() and (m["D"][em] > 0).all()
    assert not differing((m["gb"]["albedo"] * m["D"]).astype(F), m["color"])[em].any()


@pytest.mark.parametrize("J", [1, 8])
def test_the_furnace_splits_into_ambient_and_one(J):
    W, H = 48, 27
    m = sh.split_model("traced", "furnace", W, H, J, noise=0.0, ambient=1.0)
    cast = m["info"]["cast"]
    assert cast.sum() > 200 and (m["I"][cast] == F(1.0)).all() and (m["D"][cast] == F(1.0)).all()      # D = ambient + vis * 0
    em = m["info"]["emitter"]
    assert em.sum() > 200 and (m["D"][em] == F(2.0)).all() and (m["I"].view(np.uint32)[em] == 0).all()


RECOMPOSE = [("edge", n, 67, 41) for n in sh.EDGE] + [("rec", "cornell", 96, 96), ("traced", "furnace", 48, 27), ("made", "stage", 67, 41)]


@pytest.mark.parametrize("noise", [0.0, 0.6, 1.0])
def test_the_recomposed_frame_is_the_traced_frame_up_to_rounding(noise):
    """|alb (D + I) - colour| <= 10 * 2^-24 * |colour| + 2^-140 on every pixel and channel, fireflies on.
    Derivation.  colour = ((alb (first + ind)) mult) chroma, four roundings; the recomposed value rounds first mult, its product with
    chroma, ind mult, its product with chroma, the sum and the product with alb: at most four roundings on any path from an input to
    the result too.  For noise <= 1, mult >= 0 and chroma > 0, and alb, first, ind >= 0: every term is non-negative, nothing cancels,
    so each side is the exact value times (1 + e)^4 at most, e = 2^-24, and the two differ by at most ((1 + e)^4 - (1 - e)^4) ~ 8 e
    relative; 10 e leaves room for the second-order terms.  The floor covers products that fall into the denormals, where a rounding
    is absolute (2^-149 each, through at most a few factors below 8)."""
    worst = 0.0
    for kind, name, W, H in RECOMPOSE:
        amb = 1.0 if name == "furnace" else 0.15
        m = _case(kind, name, W, H, 3, noise=noise, ambient=amb)
        got = spm.compose(m["gb"]["albedo"], m["D"], m["I"]).astype(np.float64)
        col = m["color"].astype(np.float64)
        ok = np.isfinite(col)
        err = np.abs(got - col)[ok]
        bound = (10.0 * 2.0 ** -24 * np.abs(col) + 2.0 ** -140)[ok]
        rel = float((err / np.maximum(np.abs(col[ok]), 1e-30)).max()) / 2.0 ** -24
        worst = max(worst, rel)
        print(f"{name}, noise {noise}: {int(ok.sum())} values, worst error {rel:.2f} x 2^-24 of the colour (allowed 10)")
        assert np.array_equal(np.isnan(got), np.isnan(col)) and (err <= bound).all()
    assert worst > 0 or noise == 0.0


# ---- CPU 3: what examples/split_scene.cpp measures, on the oracle ---------------------------------------------------------------------
def test_two_denoised_terms_recomposed_beat_the_noisy_frame_after_eight_static_frames(pkg, orc):
    """f17's CPU experiment (64x36, noise 0, eight frames of the example's room at rest, one bounce sample and one shadow ray, against
    8 samples x 64 shadow rays averaged over 16 seeds), with each term through an oracle context of its own (sepcolor 1, addcolor 0)
    and the results recomposed.  The gate is the issue's: the recomposed frame is not worse than the noisy one in PSNR and in SSIM.
    Recorded on the last frame: noisy 11.23 dB / SSIM 0.5195, one image 19.72 dB / 0.6600, two images 19.70 dB / 0.6591: level
    with the one-image pipeline on this scene, where nothing distinguishes the settings of the two contexts."""
    import quality_model as qm
    from temporal_harness import scales
    W, H, N = 64, 36, 8
    geoms, cam, lk = sh.example_scene()
    p1 = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    p2 = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, sepcolor=1, addcolor=0)
    for p in (p1, p2):
        p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, W, H)
    first = sm.render(W, H, 0, cam, geoms, None, None, None, None, None, None, lk["centre"], seed=7, noise=0.0, fireflies=0.0)
    em = ssm.emitter_mask(W, H, cam, geoms, None, None, None)
    emit = spm.emittance_plane(W, H, cam, geoms, None, None, None)
    args = (cam, geoms, None, None, None, None, None, None)
    frame = lambda f, J, samples: stm.render(W, H, f, *args, ssm.light(samples=samples, **lk), stm.params(J, 0.15, 1), seed=7, noise=0.0,   # noqa: E731
                                             fireflies=0.0, first=first, emitters=em)
    oa, od, oi = (orc.Oracle(pkg, W, H, threads=4) for _ in range(3))
    try:
        for f in range(N):
            traced = frame(f, 1, 1)
            D, I, noisy, gb, _ = spm.render(W, H, f, *args, ssm.light(samples=1, **lk), stm.params(1, 0.15, 1), seed=7, noise=0.0,     # noqa: E741
                                            fireflies=0.0, traced=traced, emittance=emit)
            one = oa.denoise(noisy, gb, cam, p1).reshape(H, W, 3)
            fd, fi = od.denoise(D, gb, cam, p2).reshape(H, W, 3), oi.denoise(I, gb, cam, p2).reshape(H, W, 3)
    finally:
        oa.free(); od.free(); oi.free()
    two = spm.compose((gb["albedo"] * gb["ialbedo"]).astype(F), fd, fi)
    ref = np.mean([frame(100 + k, 8, 64)[0].astype(np.float64) for k in range(16)], axis=0).astype(F)
    qn, q1, q2 = qm.meter(noisy, ref), qm.meter(one, ref), qm.meter(two, ref)
    print(f"frame {N - 1}: noisy {qn['psnr_db']:.2f} dB / SSIM {qn['mean_ssim']:.4f}, one image {q1['psnr_db']:.2f} dB / SSIM {q1['mean_ssim']:.4f}, "
          f"two images {q2['psnr_db']:.2f} dB / SSIM {q2['mean_ssim']:.4f}")
    assert q2["psnr_db"] >= qn["psnr_db"] and q2["mean_ssim"] >= qn["mean_ssim"]


# ---- GPU: the split draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", sh.SIZES)
def test_split_sizes_and_seams(pkg, W, H):
    s = sh.edge("B")[0]
    scene = sh.create(pkg, s)
    m = sh.split_model("edge", "B", W, H, 3, samples=2)
    got = sh.draw(pkg, sh.TRACED, scene, W, H, s, m["lt"], sh.trace_args(3), split=True)
    traced = sh.draw(pkg, sh.TRACED, scene, W, H, s, m["lt"], sh.trace_args(3))
    scene.free()
    sh.same(got, m, f"scene B {W}x{H}, 3 bounce samples", split=True)
    sh.same((got["color"], got["gb"]), traced, f"scene B {W}x{H}: split draw vs svgf_trace_draw")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sh.EDGE)
def test_split_edge_scene_equals_the_model_and_the_traced_draw(pkg, name):
    W, H = 67, 41
    s = sh.edge(name)[0]
    scene = sh.create(pkg, s)
    lit = 0
    for J in (0, 1, 8):
        for sec in (0, 1):
            for point in (True, False):
                m = sh.split_model("edge", name, W, H, J, sec, samples=1, point=point)
                versus = J == 8 and not point
                rgb = (J + sec) % 2 == 0 or point or versus          # out_rgb NULL on some of them
                got = sh.draw(pkg, sh.TRACED, scene, W, H, s, m["lt"], sh.trace_args(J, sec), split=True, rgb=rgb)
                sh.same(got, m, f"scene {name}, {J} bounce samples, secondary shadow {sec}, {'point' if point else 'area'} light, "
                        f"out_rgb {'given' if rgb else 'NULL'}", split=True, rgb=rgb)
                lit += int((m["I"] > 0).any(axis=-1).sum())
                if versus:
                    sh.same((got["color"], got["gb"]), sh.draw(pkg, sh.TRACED, scene, W, H, s, m["lt"], sh.trace_args(J, sec)), f"scene {name} vs svgf_trace_draw")
    scene.free()
    assert lit > 0


@pytest.mark.gpu
def test_split_cornell_furnace_and_nan_normals(pkg):
    for kind, name, W, H, J, kw in (("rec", "cornell", 96, 96, 3, {}), ("traced", "furnace", 48, 27, 3, dict(noise=0.0, ambient=1.0)),
                                    ("plain", "D", 67, 41, 3, dict(samples=2)), ("made", "stage", 67, 41, 3, dict(samples=2))):
        rec = kind == "rec"
        s = sh.scene_input(kind, name)[0]
        scene = sh.create(pkg, s)
        m = sh.split_model(kind, name, W, H, J, frame=0 if rec else FRAME, seed=1 if rec else SEED, **kw)
        args = sh.trace_args(J, ambient=kw.get("ambient", 0.15), noise=kw.get("noise", 0.6))
        got = sh.draw(pkg, sh.TRACED, scene, W, H, s, m["lt"], args, split=True, frame=0 if rec else FRAME, seed=1 if rec else SEED)
        scene.free()
        sh.same(got, m, f"{name} {W}x{H}", split=True)
        if name == "furnace":
            assert (got["I"][m["info"]["cast"]] == F(1.0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rgb", [True, False])
def test_split_planar_target(pkg, rgb):
    W, H = 67, 41
    m = sh.split_model("edge", "F_cube", W, H, 3, samples=2)
    sh.check_planar_target(pkg, sh.TRACED, sh.case(sh.edge("F_cube")[0], W, H, m["lt"], sh.trace_args(3)), m,
                           f"scene F_cube, planar target, out_rgb {'given' if rgb else 'NULL'}", forms=(True,), rgb=rgb)


@functools.lru_cache(maxsize=None)
def _block_split(f, W, H, J, noise=0.6):
    """Frame f of f15's turning block under f16's area light: the split model on the posed arrays."""
    s, tables = sh.block_inputs()
    ps = pm.posed_scene(s, tables[f])
    (col, gb), info, lt = sh.traced_block_frame(f, W, H, J, 1, noise)
    emit = spm.emittance_plane(W, H, ps["cam"], ps["geoms"], None, None, None)
    D, I, col, gb, info = spm.render(W, H, f, ps["cam"], ps["geoms"], None, None, None, None, None, None, lt, stm.params(J), seed=3, noise=noise,   # noqa: E741
                                     fireflies=0.02 if noise else 0.0, traced=(col, gb, info), emittance=emit)
    return dict(D=D, I=I, color=col, gb=gb, info=info, lt=lt)


@pytest.mark.gpu
def test_the_split_follows_the_pose(pkg):
    W, H = 96, 96
    s, tables = sh.block_inputs()
    scene = sh.create(pkg, s)
    lt = _block_split(0, W, H, 2)["lt"]
    D, I, col, gb, info = spm.render(W, H, 0, *sh.args_of(s), lt, stm.params(2), seed=3)      # the scene at rest, as uploaded     # noqa: E741
    sh.same(sh.draw(pkg, sh.TRACED, scene, W, H, s, lt, sh.trace_args(2), split=True, frame=0, seed=3), dict(D=D, I=I, color=col, gb=gb),
            "turning block, before any pose", split=True)
    scene.enable_pose(len(s["geoms"]))
    terms = []
    for f in (0, 2):
        m = _block_split(f, W, H, 2)
        scene.pose(sh.dev(tables[f]))
        sh.same(sh.draw(pkg, sh.TRACED, scene, W, H, s, m["lt"], sh.trace_args(2), split=True, frame=f, seed=3), m, f"turning block, pose {f}", split=True)
        terms.append(m)
    scene.free()
    assert int((terms[0]["I"] != terms[1]["I"]).any(axis=-1).sum()) > 50 and int((terms[0]["D"] != terms[1]["D"]).any(axis=-1).sum()) > 50


@pytest.mark.gpu
def test_eight_split_draws_queued_without_host_waits(pkg):
    W, H = 67, 41
    lt = sh.split_model("edge", "A", W, H, 2)["lt"]
    sh.check_queued(pkg, sh.TRACED, sh.case(sh.edge("A")[0], W, H, lt, sh.trace_args(2)), lambda f: sh.split_model("edge", "A", W, H, 2, frame=f),
                    "queued split draw", split=True)


@pytest.mark.gpu
def test_a_captured_split_draw_is_one_kernel_node_and_replays_the_same_bits(pkg):
    W, H = 67, 41
    m = sh.split_model("edge", "B", W, H, 3)
    sh.check_captured(pkg, sh.TRACED, sh.case(sh.edge("B")[0], W, H, m["lt"], sh.trace_args(3)), m, "split draw", split=True)


@pytest.mark.gpu
def test_every_error_code_of_the_split_draw(pkg):
    import torch
    B = pkg.binding
    s = sh.edge("B")[0]
    scene = sh.create(pkg, s)
    lib = pkg.load_split_library()
    c, p = ctypes.byref(B.SvgfCamera()), ctypes.byref(B.SvgfSynthParams())
    ok = ctypes.byref(B.SvgfSceneLight.make((0, 1, 0), (1, 0, 0), (0, 0, 1), 4))
    tp = ctypes.byref(B.SvgfTraceParams(1, 0.15, 1))
    guard = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")       # every pointer below is this buffer: a refused call writes nothing
    a = guard.data_ptr()
    f = lambda h=scene.h, d=a, i=a + 16, rgb=a, gb=a, pl=None, w=1, hh=1, cm=c, spp=p, lt=ok, t=tp: lib.svgf_trace_draw_split(   # noqa: E731
        h, d, i, rgb, gb, pl, w, hh, cm, spp, lt, t, None)
    assert f(d=None) == -1 and f(i=None) == -1 and f(d=a, i=a) == -1
    sh.check_common_refusals(B, f, (B.SvgfTraceParams, sh.BAD_TRACE))
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == F(7.0)).all()
    W, H = 7, 5
    m = sh.split_model("edge", "B", W, H, 3)
    sh.same(sh.draw(pkg, sh.TRACED, scene, W, H, s, m["lt"], sh.trace_args(3), split=True), m, "after the refused calls", split=True)
    scene.free()


# ---- GPU: the recomposition ------------------------------------------------------------------------------------------------------------
# The grid is not capped (one thread per group of four pixels, at most 2^27 / 4 groups): there is no second grid-stride turn to reach.
# 67 x 41 = 2747 pixels is 686 groups: three blocks of the 16-byte path; the four sh.SIZES stay inside one.
COMPOSE_SIZES = sh.SIZES + [(67, 41)]


@functools.lru_cache(maxsize=None)
def _compose_inputs(W, H, special):
    rng = np.random.default_rng(1000 * W + H)
    n = W * H
    D, I = (rng.uniform(0.0, 4.0, (n, 3)).astype(F) for _ in range(2))      # noqa: E741
    gb = np.zeros(n, dtype=_gbuffer_dtype())
    gb["albedo"], gb["ialbedo"] = rng.uniform(0.0, 1.0, (n, 3)).astype(F), rng.uniform(0.5, 2.0, (n, 3)).astype(F)
    gb["normal"], gb["position"], gb["geomId"] = F(np.nan), F(np.inf), -7          # never read
    if special:
        v = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0, 1e-42, -3e-45, 3e38, 0.0], F)
        for arr in (D, I, gb["albedo"]):
            k = rng.integers(0, arr.size, size=max(arr.size // 3, 1))
            arr.reshape(-1)[k] = v[rng.integers(0, len(v), size=len(k))]
    a = (gb["albedo"] * gb["ialbedo"]).astype(F)
    want = spm.compose(a, D, I)
    for x in (D, I, gb, a, want):
        x.setflags(write=False)
    return D, I, gb, a, want


def _gbuffer_dtype():
    import __graft_entry__ as ge
    return ge.load_package().synth.GBUFFER_DTYPE


def _offset_dev(a, offset_floats=0):
    """The array on the device, `offset_floats` floats behind a 16-byte boundary."""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.zeros((flat.numel() + 4,), dtype=flat.dtype, device="cuda")
    view = buf[offset_floats:offset_floats + flat.numel()]
    view.copy_(flat)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * offset_floats
    return view


def _run_compose(pkg, W, H, special=False, layout="aos", off=(0, 0, 0, 0), alias=None, stream=None, twice=False):
    """off: floats behind a 16-byte boundary of (out, direct, indirect, albedo plane); alias: None, "direct" or "indirect"."""
    import torch
    D, I, gb, a, want = _compose_inputs(W, H, special)      # noqa: E741
    d, i = _offset_dev(np.array(D), off[1]), _offset_dev(np.array(I), off[2])
    out = {"direct": d, "indirect": i}.get(alias)
    if out is None:
        out = _offset_dev(np.full_like(D, np.nan), off[0])
    if layout == "aos":
        keep = torch.from_numpy(np.ascontiguousarray(gb).view(np.uint8).reshape(-1).copy()).cuda()
        g = pkg.binding.guide(gbuffer=keep)
    else:
        keep = _offset_dev(np.array(a), off[3])
        g = pkg.binding.guide(albedo=keep)
    torch.cuda.synchronize()
    for _ in range(2 if twice and alias is None else 1):
        pkg.trace_compose(out, d, i, g, W, H, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    got = out.cpu().numpy().reshape(-1, 3)
    bad = int(np.count_nonzero(differing(got[None], want[None])))
    return bad, got


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", COMPOSE_SIZES)
@pytest.mark.parametrize("layout", ["aos", "planar"])
def test_compose_equals_the_model(pkg, W, H, layout):
    for special in (False, True):
        for off in ((0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (0, 1, 0, 0), (2, 2, 2, 0)):      # 4 and 12 bytes off; mixed: the dword path
            bad, _ = _run_compose(pkg, W, H, special, layout, off)
            print(f"{W}x{H} {layout} offsets {off} special {special}: {bad} pixels differ (allowed 0)")
            assert bad == 0
        for alias in ("direct", "indirect"):
            bad, _ = _run_compose(pkg, W, H, special, layout, (1, 1, 1, 1), alias=alias)
            assert bad == 0, f"out aliasing {alias}"


@pytest.mark.gpu
def test_compose_twice_and_on_another_stream(pkg):
    import torch
    W, H = 67, 41
    st = sh.OwnStream()
    for layout in ("aos", "planar"):
        assert _run_compose(pkg, W, H, True, layout, twice=True)[0] == 0
        torch.cuda.synchronize()
        assert _run_compose(pkg, W, H, True, layout, (3, 3, 3, 3), stream=st, twice=True)[0] == 0
    st.close()


@pytest.mark.gpu
def test_a_captured_compose_is_one_kernel_node(pkg):
    import torch
    W, H = 67, 41
    D, I, gb, a, want = _compose_inputs(W, H, True)      # noqa: E741
    st = sh.OwnStream()
    d, i, out = torch.from_numpy(np.array(D)).cuda(), torch.from_numpy(np.array(I)).cuda(), torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    tex = torch.from_numpy(np.ascontiguousarray(gb).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    record = lambda: pkg.trace_compose(out, d, i, tex, W, H, stream=st)      # noqa: E731
    record()
    st.synchronize()
    graph = sh.Captured(st, record)
    with torch.cuda.stream(st.torch):
        out.zero_()
    graph.launch()
    st.synchronize()
    got = out.cpu().numpy()
    graph.destroy()
    st.close()
    assert graph.types == [0], graph.types
    assert not differing(got[None], want[None]).any()


# ---- GPU: end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pose_split_draw_two_denoises_compose_sequence(pkg, orc):
    """128x72, four frames of the turning block on one stream: pose -> split draw (1 bounce sample, 1 shadow ray) -> svgf_denoise of
    each term in a context of its own (temporal pass, sepcolor 1 / addcolor 0, the object motion table on; the f8 firefly filter on the
    indirect context only) -> svgf_trace_compose.  Each context against tests/temporal_model.py behind tests/firefly_model.py, the
    composed image against compose() of the two outputs, all on bits."""
    W, H, N = 128, 72, 4
    sh.run_split_denoise_compose(pkg, orc, sh.TRACED, [_block_split(f, W, H, 1) for f in range(N)], W, H, sh.trace_args(1),
                                 ("direct context", "indirect context, firefly filter on"), form="filtered")
